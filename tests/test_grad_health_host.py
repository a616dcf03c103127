"""Host side of the gradient-health feature, no GPU: the statistics groups of a model, the Trainer's argument checks, the logger record."""
import json
import math

import pytest
import torch


def _small_model():
    """The small CPU model of test_host_abi.test_checkpoint_dictionary_layout."""
    from Utils import configs
    from models import model_config2
    over = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
                VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8)
    mcfg = dict(configs.model_configs, **over)
    return model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg))


def test_health_groups_names_order_and_cover():
    from hdmoe_hip.optim import health_groups
    model = _small_model()
    net = model.net
    names, group_of = health_groups(model)
    E, V = len(net.Unet_experts), len(net.VIT_experts)
    want = [f"Unet_experts.{e}" for e in range(E)] + [f"VIT_experts.{e}" for e in range(V)] + ["Unet_router", "vit_router", "cross_attn"]
    if getattr(net, "scaling_net", None) is not None:
        want.append("scaling_net")
    assert names == want + ["other"] and E > 1 and V > 1
    params = list(model.parameters())
    assert len(group_of) == len(params) and all(isinstance(g, int) and 0 <= g < len(names) for g in group_of)   # exactly one group each
    where = {id(p): names[g] for p, g in zip(params, group_of)}
    for e, expert in enumerate(net.Unet_experts):
        assert {where[id(p)] for p in expert.parameters()} == {f"Unet_experts.{e}"}
    for e, expert in enumerate(net.VIT_experts):
        assert {where[id(p)] for p in expert.parameters()} == {f"VIT_experts.{e}"}
    for name in ("Unet_router", "vit_router", "cross_attn"):
        assert {where[id(p)] for p in getattr(net, name).parameters()} == {name}
    named = {id(p) for m in (net.Unet_experts, net.VIT_experts, net.Unet_router, net.vit_router, net.cross_attn) for p in m.parameters()}
    if getattr(net, "scaling_net", None) is not None:
        named |= {id(p) for p in net.scaling_net.parameters()}
    rest = [p for p in params if id(p) not in named]
    assert rest and all(where[id(p)] == "other" for p in rest)
    assert health_groups(net)[0] == names                                # the bare network gives the same groups


def test_health_groups_refuses_more_than_64():
    from hdmoe_hip.optim import health_groups

    class Wide(torch.nn.Module):
        def __init__(self, n):
            super().__init__()
            self.Unet_experts = torch.nn.ModuleList([torch.nn.Linear(2, 2) for _ in range(n)])
            self.VIT_experts = torch.nn.ModuleList([torch.nn.Linear(2, 2) for _ in range(n)])
            self.Unet_router, self.vit_router, self.cross_attn = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)

    assert len(health_groups(Wide(30))[0]) == 64                         # 60 experts + 3 + other
    with pytest.raises(ValueError, match="64"):
        health_groups(Wide(31))


class _Untouchable:
    """Stands in for the model: any attribute access is a failure of "checked before the model is touched"."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched (.{name}) before the arguments were checked")


BAD = [dict(skip_nonfinite=1), dict(skip_nonfinite="yes"), dict(skip_nonfinite=True, fuse_clip_into_step=False),
       dict(health_every=0), dict(health_every=True), dict(health_every=2.0), dict(health_every="3"),
       dict(skip_nonfinite=True, health_every=1, max_skips_in_a_row=0), dict(skip_nonfinite=True, health_every=1, max_skips_in_a_row=True),
       dict(skip_nonfinite=True, health_every=1, max_skips_in_a_row=1.5),
       dict(health_every=1, max_skips_in_a_row=2), dict(skip_nonfinite=True, max_skips_in_a_row=2), dict(max_skips_in_a_row=2)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v!r}" for k, v in kw.items()) for kw in BAD])
def test_trainer_argument_errors_come_before_the_model_is_touched(kw):
    from Utils import configs, training
    with pytest.raises(ValueError, match="Trainer: "):
        training.Trainer(_Untouchable(), configs.model_configs, configs.optim_configs, configs.loss_configs, configs.mask_configs,
                         configs.zeta_configs, **kw)


def _block(vals_norm, nonfinite):
    n = len(vals_norm)
    return {"norm": list(vals_norm), "rms": [v / 2 for v in vals_norm], "absmax": [abs(v) for v in vals_norm], "mean": [0.0] * n,
            "nonfinite": list(nonfinite), "numel": [10] * n,
            "total": {"norm": 1.0, "rms": 0.5, "absmax": 1.0, "mean": 0.0, "nonfinite": sum(nonfinite), "numel": 10 * n}}


def test_log_health_record_keys_and_nan_as_null(tmp_path):
    from graphs.logger import Logger
    lg = Logger(log_dir=str(tmp_path), run_name="run")
    names = ["Unet_experts.0", "Unet_experts.1", "other"]
    health = {"ok": 0, "measured": 5, "skipped": 2, "skipped_in_a_row": 1, "last_skipped_step": 4, "groups": names, "grad_norm": 3.5,
              "grad": _block([1.0, float("nan"), 2.0], [0, 1, 0]), "param": _block([4.0, 5.0, float("inf")], [0, 0, 0])}
    health["param"]["rms"][2] = float("nan")
    lg.log_health(4, health, names)
    lg.log_health(5, dict(health, ok=1, grad_norm=float("nan")), names)
    lines = (tmp_path / "run_health.jsonl").read_text().splitlines()
    assert len(lines) == 2 and "NaN" not in lines[0] + lines[1] and "Infinity" not in lines[0] + lines[1]
    rec = json.loads(lines[0])
    assert set(rec) == {"step", "ok", "measured", "skipped", "skipped_in_a_row", "last_skipped_step", "grad_norm", "groups", "per_group"}
    assert set(rec["per_group"]) == {"grad_norm", "grad_absmax", "grad_nonfinite", "weight_rms", "weight_absmax", "weight_nonfinite"}
    assert (rec["step"], rec["ok"], rec["measured"], rec["skipped"], rec["skipped_in_a_row"], rec["last_skipped_step"]) == (4, 0, 5, 2, 1, 4)
    assert rec["groups"] == names and rec["grad_norm"] == 3.5
    assert rec["per_group"]["grad_norm"] == [1.0, None, 2.0] and rec["per_group"]["grad_nonfinite"] == [0, 1, 0]
    assert rec["per_group"]["weight_rms"] == [2.0, 2.5, None] and rec["per_group"]["weight_absmax"] == [4.0, 5.0, None]
    assert json.loads(lines[1])["grad_norm"] is None and json.loads(lines[1])["ok"] == 1
    assert all(isinstance(v, float) and math.isfinite(v) for v in rec["per_group"]["grad_absmax"] if v is not None)
