"""Host side of the held-out evaluation (Utils/evaluation.py, graphs/logger.py Logger.log_evaluation, the two entry points in
include/hdmoe.h): the default sigma levels against closed forms, the rank slices, the argument checks, the logger's record and the
binding table.  No GPU."""
import json
import math
import re
import types

import numpy as np
import pytest
import torch


def test_default_levels_are_the_mid_quantiles_of_the_log_normal():
    from Utils.evaluation import default_levels
    pm, ps = -0.4, 1.0
    wide = dict(sigma_min=1e-30, sigma_max=1e30)
    assert default_levels(1, pm, ps, **wide) == [pytest.approx(math.exp(pm), rel=1e-15)]         # Phi^-1(1/2) = 0
    for K in (2, 3, 16, 64):
        s = default_levels(K, pm, ps, **wide)
        assert len(s) == K and all(a < b for a, b in zip(s, s[1:])), K                             # strictly monotone
        logs = np.log(s) - pm
        assert np.allclose(logs, -logs[::-1], rtol=0, atol=1e-12), K                               # symmetric about p_mean in log space
        # level k sits at percentile (k + 1/2) / K: Phi((ln s - p_mean) / p_std) through erf
        pct = [0.5 * (1 + math.erf(v / (ps * math.sqrt(2)))) for v in logs]
        assert np.allclose(pct, (np.arange(K) + 0.5) / K, rtol=0, atol=1e-12), K
    s = default_levels(16, pm, ps, sigma_min=0.3, sigma_max=2.0)
    assert min(s) == 0.3 and max(s) == 2.0 and all(a <= b for a, b in zip(s, s[1:]))               # clamped, still ordered
    assert default_levels(3, 1.5, 0.25, **wide)[1] == pytest.approx(math.exp(1.5), rel=1e-15)


@pytest.mark.parametrize("N", [1, 7, 10])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_slices_cover_the_items_disjointly(N, world):
    from Utils.evaluation import rank_slice
    seen = []
    for rank in range(world):
        first, count = rank_slice(N, world, rank)
        assert count >= 0 and first == len(seen)                                                    # contiguous, in rank order
        seen += list(range(first, first + count))
    assert seen == list(range(N))
    sizes = [rank_slice(N, world, r)[1] for r in range(world)]
    assert max(sizes) - min(sizes) <= 1


def _fake_dataset(N=10, text=True):
    """A LatentDataset without its constructor (which needs a GPU): the evaluator's checks read attributes only."""
    from Utils.utils import LatentDataset
    ds = LatentDataset.__new__(LatentDataset)
    ds.mean, ds.std = torch.zeros(N, 4, 16, 16), None
    ds.text = torch.zeros(N, 5, 32) if text else None
    ds.text_index, ds.scale, ds.flip, ds.N, ds.device = None, 1.0, 0.0, N, torch.device("cpu")
    return ds


class _Model(torch.nn.Module):
    def forward(self, x, sigma, text_emb, Unet_router_mask, Vit_router_mask, zeta, transition_point, softness, return_log_var=False):
        raise AssertionError("an argument check ran the model")


def _make(**kw):
    from Utils import configs
    from Utils.evaluation import Evaluator
    args = dict(model=_Model(), model_config=configs.model_configs, mask_config=configs.mask_configs, dataset=_fake_dataset(), batch_size=4)
    args.update(kw)
    return Evaluator(args.pop("model"), args.pop("model_config"), args.pop("mask_config"), args.pop("dataset"), args.pop("batch_size"), **args)


def test_argument_checks_raise_value_error_without_a_gpu():
    from Utils import configs
    ev = _make(levels=3, rounds=3, seed=5, world=2, rank=1)
    assert ev.K == 3 and (ev.first, ev.n_rank) == (5, 5) and ev.buf is None
    assert ev._model_extra == {"transition_point": configs.mask_configs["p_mean"], "softness": configs.mask_configs["p_std"],
                               "return_log_var": True}
    assert _make(levels=[0.5, 2.0]).sigmas == [0.5, 2.0]                                           # a sequence is used as given
    bad = [("dataset", dict(dataset="flowers")), ("text", dict(dataset=_fake_dataset(text=False))), ("batch_size", dict(batch_size=0)),
           ("batch_size", dict(batch_size=4097)), ("batch_size", dict(batch_size=2.0)), ("levels", dict(levels=0)), ("levels", dict(levels=65)),
           ("levels", dict(levels=[])), ("levels", dict(levels=[1.0, -1.0])), ("levels", dict(levels=[float("nan")])),
           ("levels", dict(levels=[1.0] * 65)), ("levels", dict(levels=True)), ("levels", dict(levels="abc")),
           ("rounds", dict(levels=3, rounds=0)), ("rounds", dict(levels=3, rounds=4)), ("seed", dict(seed=1.5)),
           ("null_text_emb", dict(null_text_emb=[0.0])), ("null_text_emb", dict(null_text_emb=torch.zeros(5, 31))),
           ("ema", dict(ema=object())), ("world", dict(world=2)), ("rank", dict(world=2, rank=2)), ("world", dict(world=0, rank=0))]
    for name, kw in bad:
        with pytest.raises(ValueError, match=name):
            _make(**kw)
    with pytest.raises(ValueError, match="text"):
        ev.evaluate(text="uncond")
    with pytest.raises(ValueError, match="profile"):
        ev.evaluate(profile=0)                                                                     # no ema
    fake_ema = types.SimpleNamespace(swapped=None, nprofiles=2)
    with pytest.raises(ValueError, match="profile"):
        _make(ema=fake_ema).evaluate(profile=2)
    assert ev.buf is None                                                                          # nothing was allocated


def test_trainer_keywords_validate_like_ema_snapshot_every():
    """Before the optimizer is built: a model without the expected structure is never looked at."""
    from Utils import configs, training
    mk = lambda **kw: training.Trainer(_Model(), configs.model_configs, configs.optim_configs, configs.loss_configs, configs.mask_configs,
                                       configs.zeta_configs, **kw)
    ev = types.SimpleNamespace(evaluate=lambda **kw: None)
    for kw in (dict(eval_every=1), dict(evaluator=ev), dict(evaluator=ev, eval_every=0), dict(evaluator=ev, eval_every=1.5),
               dict(evaluator=ev, eval_every=True), dict(evaluator=object(), eval_every=1)):
        with pytest.raises(ValueError, match="eval"):
            mk(**kw)


def test_summarize_means_stderr_and_empty_levels():
    from Utils.evaluation import summarize
    E = 2
    acc = np.zeros((3, 6 + 4 * E))
    mses = np.array([1.0, 2.0, 4.0, 5.0])
    acc[0, :6] = [4, mses.sum(), (mses ** 2).sum(), 2 * mses.sum(), 3.0, -2.0]
    acc[0, 6:] = [2.0, 1.0, 4, 2, 3.0, 0.0, 4, 0]
    acc[2, :6] = [1, 7.0, 49.0, 7.0, 7.0, 0.0]
    r = summarize(acc, [0.1, 1.0, 10.0], E)
    assert r["count"].tolist() == [4, 0, 1] and r["n"] == 5 and r["mse_mean"] == pytest.approx((mses.sum() + 7.0) / 5)
    assert r["mse"][0] == 3.0 and math.isnan(r["mse"][1]) and r["mse"][2] == 7.0
    assert r["mse_stderr"][0] == pytest.approx(math.sqrt(mses.var() / 4)) and math.isnan(r["mse_stderr"][1]) and r["mse_stderr"][2] == 0.0
    assert r["edm_weighted"][0] == 6.0 and r["nll"][0] == 0.75 and r["log_var"][0] == -0.5
    assert r["unet_usage"][0].tolist() == [0.5, 0.25] and r["unet_selected"][0].tolist() == [1.0, 0.5]
    assert r["vit_usage"][0].tolist() == [0.75, 0.0] and r["vit_selected"][0].tolist() == [1.0, 0.0]
    assert np.isnan(r["unet_usage"][1]).all() and np.array_equal(r["acc"], acc)
    for key in ("sigma", "count", "mse", "mse_stderr", "edm_weighted", "nll", "log_var"):
        assert r[key].dtype == np.float64 and r[key].shape == (3,), key
    for key in ("unet_usage", "vit_usage", "unet_selected", "vit_selected"):
        assert r[key].dtype == np.float64 and r[key].shape == (3, E), key


def test_logger_writes_one_validation_record(tmp_path, capsys):
    from Utils.evaluation import summarize
    from graphs.logger import Logger
    E = 2
    acc = np.zeros((2, 6 + 4 * E))
    acc[0] = [2, 3.0, 5.0, 6.0, 3.0, 0.0, 1.0, 1.0, 2, 2, 0.5, 1.5, 1, 2]
    res = summarize(acc, [0.5, 2.0], E)
    lg = Logger(log_dir=str(tmp_path), run_name="run")
    capsys.readouterr()
    before = sorted(p.name for p in tmp_path.iterdir())
    lg.log_evaluation(7, res)
    lg.log_evaluation(7, res, tag="ema0")
    path = tmp_path / "run_validation.jsonl"
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(before + ["run_validation.jsonl"])
    recs = [json.loads(line) for line in path.read_text().splitlines()]
    assert [r["tag"] for r in recs] == ["raw", "ema0"] and all(r["step"] == 7 for r in recs)
    keys = {"step", "tag", "mse_mean", "n", "sigma", "count", "mse", "mse_stderr", "edm_weighted", "nll", "log_var", "unet_usage", "vit_usage",
            "unet_selected", "vit_selected"}
    assert set(recs[0]) == keys
    assert recs[0]["count"] == [2.0, 0.0] and recs[0]["mse"] == [1.5, None] and recs[0]["n"] == 2.0        # an empty level: null, valid JSON
    assert recs[0]["unet_usage"] == [[0.5, 0.5], [None, None]] and recs[0]["sigma"] == [0.5, 2.0]


def test_header_declares_the_entry_points_and_the_binding_has_them():
    from hdmoe_hip import _lib
    assert _lib.SIGNATURES["hdmoe_eval_inputs"] == "pppppp" + "i" + "p" + "u" + "i" + "lllll" + "i" + "d" + "s"
    assert _lib.SIGNATURES["hdmoe_eval_accumulate"] == "ppppppppp" + "i" + "l" + "ii" + "d" + "s"
    assert _lib.SIGNATURES["hdmoe_eval_chunk"] == ""
    text = open(_lib.HEADER_PATH).read()
    salts = {int(m, 16) for m in re.findall(r"\^ (0x[0-9A-F]{16})", text)}
    from hdmoe_hip import ops
    assert ops.EVAL_SALT in salts and ops.EVAL_SALT & 1 and len(salts) >= 3                        # a third XOR constant, odd


def test_eval_report_prints_the_table_and_both_maps(tmp_path, capsys):
    import importlib.util
    import os
    from Utils.evaluation import summarize
    from graphs.logger import Logger
    spec = importlib.util.spec_from_file_location("eval_report", os.path.join(os.path.dirname(__file__), "..", "tools", "eval_report.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    E = 2
    acc = np.zeros((3, 6 + 4 * E))
    acc[0] = [2, 3.0, 5.0, 6.0, 3.0, 0.0, 1.0, 1.0, 2, 2, 0.5, 1.5, 1, 2]
    acc[2] = [1, 0.25, 0.0625, 1.0, 0.25, 0.0, 0.0, 1.0, 0, 1, 1.0, 0.0, 1, 0]
    lg = Logger(log_dir=str(tmp_path), run_name="run")
    for step in (1, 2):
        lg.log_evaluation(step, summarize(acc * step, [0.1, 1.0, 10.0], E))
        lg.log_evaluation(step, summarize(acc, [0.1, 1.0, 10.0], E), tag="ema0")
    capsys.readouterr()
    path = str(tmp_path / "run_validation.jsonl")
    assert tool.main([path]) == 0
    out = capsys.readouterr().out
    assert out.count("step 2") == 2 and "step 1" not in out and "tag raw" in out and "tag ema0" in out     # the last step, every tag
    assert out.count("U-Net router, mean gate probability") == 2 and out.count("ViT router, mean gate probability") == 2
    assert "nan" in out                                                                                    # the empty level
    lines = [l for l in out.splitlines() if l.startswith("  e")]
    assert len(lines) == 2 * 2 * E and all(len(l.split()) >= 1 + 3 for l in lines)                         # E rows of K cells per map
    assert tool.main([path, "--step", "1", "--tag", "ema0", "--selected"]) == 0
    out = capsys.readouterr().out
    assert out.count("step 1") == 1 and "fraction of samples" in out
    assert tool.main([path, "--step", "7"]) == 1
