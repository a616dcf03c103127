"""Host-only check of what `Utils.training.Trainer.train_step` calls, in which order and with which distinguishing arguments, in the
default (host-input, eager) mode: a real Trainer over a toy model on the CPU, every collaborator replaced by a recorder.  The graphed and
device-input arms need the GPU and stay with test_trainer_graphed.py, test_trainer_cond_dropout.py and test_latent_dataset.py.

Where the literals come from: EXPECTED, SIGMA and KEEP were printed by running `record()` of this file against the Trainer of the commit
before the step bodies were folded into one (four step bodies, two capture builders), in a checkout of that commit -- not against the
code under test.  A case's record is one list per step: the calls, then ("keys", the returned dictionary's keys in order)."""
import os

import pytest
import torch

VERDICT = "verdict"                                             # stands for the fake GradHealth's `ok` tensor in a recorded argument


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        lin = lambda: torch.nn.Linear(2, 2)
        self.Unet_experts, self.VIT_experts = torch.nn.ModuleList([lin(), lin()]), torch.nn.ModuleList([lin(), lin()])
        self.cross_attn, self.Unet_router, self.vit_router = lin(), lin(), lin()


class _Model(torch.nn.Module):
    def __init__(self, rec):
        super().__init__()
        self.net, self.rec = _Net(), rec
        self.net.cross_attn.weight.register_hook(lambda g: rec.append(("backward",)))

    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, return_log_var=False):
        self.rec.append(("forward",))
        one = torch.ones(x.shape[0], 2)
        return {"denoised": x * self.net.cross_attn.weight.sum(), "log_var": None, "Unet_router_loss": one, "vit_router_loss": one,
                "scaling_net_out": one, "out_gate": one}


class _Recorder:
    """Every ``log_*`` / listed method appends (prefix.name, *what tells the call apart) to the shared list."""

    def __init__(self, rec, prefix, tell, returns=None):
        self._rec, self._prefix, self._tell, self._returns = rec, prefix, tell, returns or {}

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._tell:
            raise AttributeError(name)

        def call(*a, **k):
            self._rec.append((f"{self._prefix}.{name}",) + tuple(self._tell[name](*a, **k)))
            return self._returns.get(name)
        return call


def _ok(k, health):
    return VERDICT if k.get("ok") is health.ok else k.get("ok")


class _Health:
    def __init__(self, rec, skipped_in_a_row=0):
        self.rec, self.skipped = rec, skipped_in_a_row
        self.ok, self.total_sumsq = torch.ones(1, dtype=torch.int32), torch.full((1,), 4.0)

    def measure(self, step, which="grad", verdict=True):
        self.rec.append(("health.measure", step, which, verdict))

    def read(self):
        self.rec.append(("health.read",))
        return {"groups": ["g"], "param": {"total": {"nonfinite": 0}, "nonfinite": [0]}, "skipped_in_a_row": self.skipped, "last_skipped_step": 1}


class _Evaluator:
    def __init__(self, rec, ema):
        self.rec, self.ema = rec, ema

    def evaluate(self, profile=None):
        self.rec.append(("evaluator.evaluate", profile))
        return {"profile": profile}


LOGGER = {"log_training_step": lambda **k: (k["step"],), "log_router_statistics": lambda **k: (k["step"],), "log_scaling_gating": lambda **k: (),
          "log_gradients": lambda **k: (k["step"],), "log_weight_statistics": lambda **k: (k["step"],),
          "log_health": lambda step, h, groups: (step,), "log_evaluation": lambda step, r, tag: (step, tag),
          "log_balance": lambda step, b: (step, b)}

# name -> (Trainer keywords, what is attached behind the constructor, steps)
CASES = {
    "default": (dict(), (), 2),
    "unfused_clip": (dict(fuse_clip_into_step=False), (), 1),
    "logger": (dict(), ("logger",), 1),
    "ema_snapshot_every_2": (dict(ema_snapshot_every=2), ("ema",), 2),
    "skip_nonfinite": (dict(skip_nonfinite=True), ("health", "ema"), 1),
    "health_every_2_observe_only": (dict(health_every=2), ("health", "logger"), 2),
    "health_every_2_skip_nonfinite": (dict(health_every=2, skip_nonfinite=True), ("health", "logger"), 2),
    "max_skips_in_a_row": (dict(health_every=1, skip_nonfinite=True, max_skips_in_a_row=3), ("health3",), 1),
    "balance": (dict(), ("balance",), 1),
    "balance_skip_nonfinite": (dict(skip_nonfinite=True), ("health", "balance"), 1),
    "balance_logged_on_health_step": (dict(health_every=2), ("health", "balance", "logger"), 2),
    "evaluator_with_ema": (dict(eval_every=2), ("ema", "evaluator", "logger"), 2),
    "cond_dropout_host": (dict(cond_dropout=0.5), (), 2),
}


def record(name, tmp):
    """Per step of case `name`: the recorded calls and the keys of the result (or the exception's type); and the trainer's results."""
    import hdmoe_hip.optim as hoptim
    from Utils import configs, training
    kw, attach, steps = CASES[name]
    rec = []
    torch.manual_seed(1234)
    model = _Model(rec)
    ema = evaluator = None
    if "ema" in attach:
        ema = _Recorder(rec, "ema", {"update": lambda **k: (_ok(k, health),), "save_snapshot": lambda path: (os.path.relpath(path, tmp),)})
        ema.__dict__["nprofiles"] = 2
        if "ema_snapshot_every" in kw:
            kw = dict(kw, ema_snapshot_dir=os.path.join(tmp, "snap"))
    if "evaluator" in attach:
        evaluator = _Evaluator(rec, ema)
    logger = _Recorder(rec, "logger", LOGGER) if "logger" in attach else None
    mcfg = dict(configs.model_configs, num_experts=2)
    mask = dict(configs.mask_configs, unet_attr=[0.0, 1.0], vit_attr=[1.0, 0.0])
    tr = training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, mask, configs.zeta_configs, logger=logger, ema=ema,
                          evaluator=evaluator, **kw)
    health = _Health(rec, skipped_in_a_row=3 if "health3" in attach else 0)
    if "health" in attach or "health3" in attach:
        tr._health = health
    if "balance" in attach:
        tr.balance = _Recorder(rec, "balance", {"step": lambda **k: (_ok(k, health),), "last": lambda: (), "read": lambda: (), "clear": lambda: ()},
                               returns={"last": "LAST", "read": "READ"})
    tr.criterion = lambda sigma_vec, x, sigma, out_model: {"loss": (out_model["denoised"] - x).square().mean(), "denoising": 0.0, "balance": 0.0,
                                                           "z_loss": 0.0, "entropy": 0.0, "pure_loss": 0.0}
    tr.optimizer.step = lambda *a, **k: rec.append(("optimizer.step", k.get("clip") is not None and k["clip"][1], k.get("health") is health))
    tr.scheduler.step = lambda: rec.append(("scheduler.step",))
    for meth in ("zero_grad", "finish"):
        def wrapped(inner=getattr(tr.buckets, meth), meth=meth):
            rec.append((f"buckets.{meth}",))
            return inner()
        setattr(tr.buckets, meth, wrapped)
    clip_was = hoptim.clip_grad_norm_
    hoptim.clip_grad_norm_ = lambda params, max_norm: rec.append(("clip_grad_norm_", max_norm))
    try:
        lat, text = torch.randn(4, 2, 3, 3), torch.randn(4, 3, 5)
        out, results = [], []
        for _ in range(steps):
            del rec[:]
            try:
                res = tr.train_step(lat, text)
                out.append(list(rec) + [("keys",) + tuple(res)])
                results.append(res)
            except RuntimeError as exc:
                out.append(list(rec) + [("raised", type(exc).__name__, str(exc)[:40])])
        assert tr.step_idx == steps
    finally:
        hoptim.clip_grad_norm_ = clip_was
    return out, results, tr


F, BWD = [("forward",)], [("buckets.zero_grad",), ("backward",), ("buckets.finish",)]
KEYS = ("keys", "loss", "out_model", "sigma")
OPT, OPT_GUARDED, SCHED = ("optimizer.step", 1.0, False), ("optimizer.step", 1.0, True), ("scheduler.step",)   # (name, clip's max_norm, health given)
LOG_F = lambda s: [("logger.log_training_step", s), ("logger.log_router_statistics", s), ("logger.log_scaling_gating",)]
LOG_G = lambda s: [("logger.log_gradients", s), ("logger.log_weight_statistics", s)]
READ = lambda s: [("health.measure", s, "param", False), ("health.read",)]
EVAL = [("evaluator.evaluate", None), ("evaluator.evaluate", 0), ("evaluator.evaluate", 1),
        ("logger.log_evaluation", 2, "raw"), ("logger.log_evaluation", 2, "ema0"), ("logger.log_evaluation", 2, "ema1")]

EXPECTED = {
    "default": [F + BWD + [OPT, SCHED, KEYS]] * 2,
    "unfused_clip": [F + BWD + [("clip_grad_norm_", 1.0), ("optimizer.step", False, False), SCHED, KEYS]],
    "logger": [F + LOG_F(0) + BWD + LOG_G(0) + [OPT, SCHED, KEYS]],
    "ema_snapshot_every_2": [
        F + BWD + [OPT, ("ema.update", None), SCHED, KEYS],
        F + BWD + [OPT, ("ema.update", None), ("ema.save_snapshot", os.path.join("snap", "ema_00000002.pt")), SCHED, KEYS]],
    "skip_nonfinite": [F + BWD + [("health.measure", 0, "grad", True), OPT_GUARDED, ("ema.update", VERDICT), SCHED, KEYS + ("step_ok", "grad_norm")]],
    "health_every_2_observe_only": [
        F + LOG_F(0) + BWD + LOG_G(0) + [OPT, SCHED, KEYS],
        F + LOG_F(1) + BWD + [("health.measure", 1, "grad", False)] + LOG_G(1) + [OPT, SCHED] + READ(2) + [("logger.log_health", 1), KEYS]],
    "health_every_2_skip_nonfinite": [
        F + LOG_F(0) + BWD + [("health.measure", 0, "grad", True)] + LOG_G(0) + [OPT_GUARDED, SCHED, KEYS + ("step_ok", "grad_norm")],
        F + LOG_F(1) + BWD + [("health.measure", 1, "grad", True)] + LOG_G(1) + [OPT_GUARDED, SCHED] + READ(2)
        + [("logger.log_health", 1), KEYS + ("step_ok", "grad_norm")]],
    "max_skips_in_a_row": [F + BWD + [("health.measure", 0, "grad", True), OPT_GUARDED, SCHED] + READ(1)
                           + [("raised", "RuntimeError", "Trainer: 3 steps in a row had non-finite")]],
    "balance": [F + BWD + [OPT, ("balance.step", None), SCHED, ("balance.last",), KEYS + ("router_balance",)]],
    "balance_skip_nonfinite": [F + BWD + [("health.measure", 0, "grad", True), OPT_GUARDED, ("balance.step", VERDICT), SCHED, ("balance.last",),
                                          KEYS + ("step_ok", "grad_norm", "router_balance")]],
    "balance_logged_on_health_step": [
        F + LOG_F(0) + BWD + LOG_G(0) + [OPT, ("balance.step", None), SCHED, ("balance.last",), KEYS + ("router_balance",)],
        F + LOG_F(1) + BWD + [("health.measure", 1, "grad", False)] + LOG_G(1) + [OPT, ("balance.step", None), SCHED] + READ(2)
        + [("logger.log_health", 1), ("balance.read",), ("logger.log_balance", 1, "READ"), ("balance.last",), KEYS + ("router_balance",)]],
    "evaluator_with_ema": [
        F + LOG_F(0) + BWD + LOG_G(0) + [OPT, ("ema.update", None), SCHED, KEYS],
        F + LOG_F(1) + BWD + LOG_G(1) + [OPT, ("ema.update", None), SCHED] + EVAL + [KEYS]],
    "cond_dropout_host": [F + BWD + [OPT, SCHED, KEYS + ("text_keep",)]] * 2,
}
# sigma (flattened) and text_keep of "cond_dropout_host"'s two steps
SIGMA = [[0.00321852695196867, 1.7706302404403687, 0.0486106351017952, 0.002951754489913583],
         [1.2487365007400513, 0.19821389019489288, 11.707100868225098, 0.1120779737830162]]
KEEP = [[1.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_train_step_makes_the_parents_calls_in_the_parents_order(name, tmp_path):
    got, results, tr = record(name, str(tmp_path))
    for step, (g, w) in enumerate(zip(got, EXPECTED[name])):
        assert g == w, (name, step)
    assert len(got) == len(EXPECTED[name])
    if name == "evaluator_with_ema":
        assert tr.last_eval == {"step": 2, "results": {"raw": {"profile": None}, "ema0": {"profile": 0}, "ema1": {"profile": 1}}}
    if name.startswith("health_every_2"):
        assert tr.last_health["groups"] == ["g"]
    if name == "balance":
        assert results[0]["router_balance"] == "LAST"
    if name == "skip_nonfinite":
        assert int(results[0]["step_ok"]) == 1 and float(results[0]["grad_norm"]) == 2.0


def test_cond_dropout_draws_from_torchs_generator_in_the_parents_order(tmp_path):
    """Dropout first, then sigma, then the noise: sigma and text_keep of two steps under torch.manual_seed(1234) are the parent's.  The
    draws are exact integers of the generator; exp() behind them may differ in the last bit between CPUs, hence 1e-5 relative (24-bit
    mantissa: 6e-8 per rounding) -- another draw order gives unrelated values."""
    _, results, _ = record("cond_dropout_host", str(tmp_path))
    for res, sigma, keep in zip(results, SIGMA, KEEP):
        assert res["text_keep"].tolist() == keep
        assert res["sigma"].flatten().tolist() == pytest.approx(sigma, rel=1e-5)
        assert tuple(res["sigma"].shape) == (4, 1, 1, 1)
