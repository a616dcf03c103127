"""Utils.evaluation.Evaluator on the small config-2 model: against a plain loop with the statistics in torch fp64, graphed against
eager, determinism, batch size, rank slices, EMA profiles, the unconditional branch, and -- the part training depends on -- that an
evaluation leaves the training state bit for bit as it found it.  The helpers are those of test_latent_dataset.py, copied so that the
file stands alone."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TINY = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
            VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8, top_k=2)
TSEED = 0x0BADC0FFEE123457
ESEED = 0x5EED0FE7A1
N, B, K = 10, 4, 3
# the kernel test's bound on what comes from the sums of squares (tests/test_eval_kernels.py: chains of 16 + 6 + 4 fp32 additions)
SSE_TOL = 4 * (16 + 6 + 4) * 2.0 ** -24


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model


def _tables():
    g = torch.Generator(device=DEV).manual_seed(3)
    mean = 0.5 * torch.randn(N, 4, 16, 16, device=DEV, generator=g)
    std = 0.1 + torch.rand(N, 4, 16, 16, device=DEV, generator=g)
    text = torch.randn(N, 5, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    return mean, std, text


def _dataset(text=None):
    from Utils.utils import LatentDataset
    mean, std, rows = _tables()
    return LatentDataset(mean, std, scale=1.0, flip=0.5, text=rows if text is None else text)


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


def _tiny_trainer(model=None, **kw):
    """The small config-2 model of test_latent_dataset.py: zeta 0 and every dropout p = 0, so a step is a function of its weights and
    inputs alone."""
    from Utils import training
    configs, mcfg, zeta = _cfgs()
    model = _model(train=True) if model is None else model
    return training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, zeta, **kw)


def _evaluator(model, ds=None, batch_size=B, **kw):
    from Utils.evaluation import Evaluator
    configs, mcfg, _ = _cfgs()
    kw = dict(dict(levels=K, rounds=K, seed=ESEED), **kw)
    return Evaluator(model, mcfg, configs.mask_configs, _dataset() if ds is None else ds, batch_size, **kw)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def shared():
    """One model and its graphed evaluation, computed once and left unchanged: the reference of several tests."""
    model = _model()
    ev = _evaluator(model)
    res = ev.evaluate()
    return model, ev, res


def test_evaluate_matches_a_plain_loop(shared):
    """rounds = K: every (item, level) pair once.  The loop makes the same batches with ops.eval_inputs, runs them through model.eval()
    one at a time and keeps the statistics in torch fp64."""
    from hdmoe_hip import ops
    from Utils import configs
    model, ev, res = shared
    _, mcfg, _ = _cfgs()
    ds = ev.dataset
    E, sd = mcfg["num_experts"], mcfg["sigma_data"]
    levels = torch.tensor(ev.sigmas, dtype=torch.float32, device=DEV)
    acc = torch.zeros(K, 6 + 4 * E, dtype=torch.float64, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    x, x0, sigma = torch.zeros(B, 4, 16, 16, **f32), torch.zeros(B, 4, 16, 16, **f32), torch.zeros(B, 1, 1, 1, **f32)
    level, item = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    pairs = set()
    assert not model.training
    for rnd in range(K):
        for first in range(0, N, B):
            count = min(B, N - first)
            ops.eval_inputs(x, x0, sigma, level, item, ds.mean, levels, ESEED, rnd, first, count, scale=ds.scale)
            with torch.no_grad():
                out = model(x=x, sigma=sigma, text_emb=ds.text[item.long()], Unet_router_mask=torch.ones(B, E, **f32),
                            Vit_router_mask=torch.ones(B, E, **f32), zeta=0.0, return_log_var=True,
                            transition_point=configs.mask_configs["p_mean"], softness=configs.mask_configs["p_std"])
            mse = (out["denoised"].double() - x0.double()).pow(2).flatten(1).mean(1)
            sg = sigma.double().view(B)
            lv = out["log_var"].double().view(B).clamp(-10, 10)
            pu, pv = out["Unet_router_loss"].double(), out["vit_router_loss"].double()
            rows = torch.cat([torch.ones(B, 1, dtype=torch.float64, device=DEV), mse[:, None], mse[:, None] ** 2,
                              ((sg ** 2 + sd ** 2) / (sg * sd) ** 2 * mse)[:, None], (mse * torch.exp(-lv) + lv)[:, None], lv[:, None],
                              pu, (pu > 0).double(), pv, (pv > 0).double()], dim=1)
            for i in range(count):
                acc[int(level[i])] += rows[i]
                pairs.add((int(item[i]), int(level[i])))
            assert level[count:].eq(-1).all()
    assert pairs == {(i, k) for i in range(N) for k in range(K)}
    ref = acc.cpu().numpy()
    got = res["acc"]
    assert res["count"].tolist() == [N] * K and res["n"] == N * K and np.array_equal(got[:, 0], ref[:, 0])
    sel = np.r_[6 + E + np.arange(E), 6 + 3 * E + np.arange(E)]
    assert np.array_equal(got[:, sel], ref[:, sel])                                                # selection counts: exact
    prob = np.r_[6 + np.arange(E), 6 + 2 * E + np.arange(E)]
    assert np.all(np.abs(got[:, prob] - ref[:, prob]) <= 1e-12 * ref[:, prob])                     # usage maps
    err = np.abs(got[:, 1:4] - ref[:, 1:4]) / ref[:, 1:4]
    print(f"mse per level {res['mse']}, worst relative gap of an SSE-derived sum {err.max():.3e} (bound {SSE_TOL:.3e})")
    assert np.all(err <= np.array([SSE_TOL, 2 * SSE_TOL, SSE_TOL]))
    assert np.allclose(res["mse"], ref[:, 1] / N, rtol=SSE_TOL, atol=0) and np.allclose(res["unet_usage"], ref[:, 6:6 + E] / N, rtol=1e-12)
    assert np.allclose(res["log_var"], ref[:, 5] / N, rtol=1e-12, atol=1e-15)
    assert res["mse_mean"] == pytest.approx(ref[:, 1].sum() / (N * K), rel=SSE_TOL)
    assert np.allclose(res["sigma"], ev.sigmas) and np.all(np.diff(res["mse"]) != 0)
    for key in ("unet_selected", "vit_selected"):
        assert np.array_equal(res[key], ref[:, sel[:E] if key[0] == "u" else sel[E:]] / N) and res[key].min() >= 0 and res[key].max() <= 1
    print(f"unet usage per level\n{res['unet_usage']}\nunet selected\n{res['unet_selected']}")


def test_graphed_equals_eager_and_repeats_bit_for_bit(shared):
    model, ev, res = shared
    assert ev.graphed and ev._step is not None
    eager = _evaluator(model, graphed=False).evaluate()
    assert np.array_equal(_bits(eager["acc"]), _bits(res["acc"]))
    again = ev.evaluate()
    assert np.array_equal(_bits(again["acc"]), _bits(res["acc"]))


def test_numbers_follow_the_weights_after_an_optimizer_step():
    """The captured batch holds no weight-prepare launch: after an optimizer step the evaluation must not read the stale images."""
    tr = _tiny_trainer(dataset=_dataset(), batch_size=B, seed=TSEED)
    ev = _evaluator(tr.model)
    a = ev.evaluate()
    b = ev.evaluate()
    assert np.array_equal(_bits(a["acc"]), _bits(b["acc"])) and tr.model.training
    tr.train_step()
    c = ev.evaluate()
    assert np.array_equal(c["acc"][:, 0], a["acc"][:, 0]) and np.all(c["acc"][:, 1] != a["acc"][:, 1])
    fresh = _evaluator(tr.model, graphed=False).evaluate()                                         # an eager pass over the new weights
    assert np.array_equal(_bits(fresh["acc"]), _bits(c["acc"]))


def test_batch_size_changes_counts_not_and_mse_within_the_fp32_bound(shared):
    """B = 4 against B = 5 in fp32 compute mode.  Tolerance: the fp32 bound on `denoised` of tests/test_bench_path_parity.py (1e-4 of the
    tensor's largest entry), doubled for the square.  Measured on an MI355X: a gap of exactly 0 on every level -- at these shapes the
    forward of a sample does not depend on the rest of its batch."""
    model, ev, res = shared
    other = _evaluator(model, batch_size=5).evaluate()
    assert np.array_equal(other["count"], res["count"]) and other["n"] == res["n"]
    gap = np.abs(other["mse"] - res["mse"]) / res["mse"]
    print(f"B = 4 vs B = 5: relative mse gap per level {gap}")
    assert np.all(gap <= 2 * 1e-4)
    for key in ("unet_selected", "vit_selected"):
        assert np.array_equal(other[key], res[key])


def test_two_ranks_sum_to_one(shared):
    """world = 2 without a process group: rank r takes a contiguous slice; the raw tables add up to the world = 1 table."""
    model, ev, res = shared
    parts = [_evaluator(model, world=2, rank=r) for r in range(2)]
    assert [(p.first, p.n_rank) for p in parts] == [(0, 5), (5, 5)]
    accs = [p.evaluate()["acc"] for p in parts]
    total = accs[0] + accs[1]
    E = (total.shape[1] - 6) // 4
    exact = np.r_[0, 6 + E + np.arange(E), 6 + 3 * E + np.arange(E)]
    assert np.array_equal(total[:, exact], res["acc"][:, exact]) and accs[0][:, 0].tolist() == [5] * K
    rest = np.setdiff1d(np.arange(total.shape[1]), exact)
    gap = np.abs(total[:, rest] - res["acc"][:, rest]) / np.abs(res["acc"][:, rest]).clip(min=1e-300)
    print(f"world 2 vs 1: worst relative gap of a sum {gap.max():.3e}")
    assert np.all(gap <= 1e-12)


def test_ema_profile_equals_a_model_filled_by_copy_to():
    from hdmoe_hip import bank
    from hdmoe_hip.ema import WeightEMA
    model = _model()
    ema = WeightEMA(model, betas=(0.5,))
    g = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():                                     # move the raw weights away from the average
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, device=DEV, generator=g))
    bank.note_weights_changed()
    ema.update()                                              # the profile: half way between the old and the new weights
    ev = _evaluator(model, ema=ema)
    raw = ev.evaluate()
    before = [p.detach().clone() for p in model.parameters()]
    prof = ev.evaluate(profile=0)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))                      # swapped back bit for bit
    assert not np.array_equal(prof["acc"][:, 1], raw["acc"][:, 1])
    other = _model()
    ema.copy_to(other, 0)
    want = _evaluator(other).evaluate()
    assert np.array_equal(_bits(prof["acc"]), _bits(want["acc"]))
    assert np.array_equal(_bits(ev.evaluate()["acc"]), _bits(raw["acc"]))                          # and the raw numbers are back


def test_null_text_equals_the_null_row_as_the_only_text_row(shared):
    model, ev, res = shared
    null = torch.randn(5, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    a = _evaluator(model, null_text_emb=null).evaluate(text="null")
    b = _evaluator(model, ds=_dataset(text=null[None])).evaluate()
    assert np.array_equal(_bits(a["acc"]), _bits(b["acc"])) and not np.array_equal(a["acc"][:, 1], res["acc"][:, 1])
    z = _evaluator(model).evaluate(text="null")                                                    # no null row: zeros
    zz = _evaluator(model, ds=_dataset(text=torch.zeros(1, 5, 32, device=DEV))).evaluate()
    assert np.array_equal(_bits(z["acc"]), _bits(zz["acc"]))
    # one evaluator, both branches in turn: the static text buffer follows
    both = _evaluator(model, null_text_emb=null)
    assert np.array_equal(_bits(both.evaluate()["acc"]), _bits(res["acc"]))
    assert np.array_equal(_bits(both.evaluate(text="null")["acc"]), _bits(a["acc"]))
    assert np.array_equal(_bits(both.evaluate()["acc"]), _bits(res["acc"]))


def _usage(model):
    return [u for u in (getattr(m, "_hdmoe_usage", None) for m in model.modules()) if torch.is_tensor(u)]


def test_a_bare_evaluate_leaves_counters_mode_and_seed_stream():
    import hdmoe_hip
    from hdmoe_hip import ops
    tr = _tiny_trainer(dataset=_dataset(), batch_size=B, seed=TSEED)
    tr.train_step()                                           # the forward installs the routed-row counters
    usage = _usage(tr.model)
    assert len(usage) == 2
    for n, u in enumerate(usage):
        u.copy_(torch.arange(1, u.numel() + 1, device=DEV) + 10.0 * n)
    saved = [u.clone() for u in usage]
    params = [p.detach().clone() for p in tr.model.parameters()]
    grads = [None if p.grad is None else p.grad.detach().clone() for p in tr.model.parameters()]
    hdmoe_hip.manual_seed(99)
    seed_state, ctr = dict(ops._seed_state), ops.step_counter(DEV).clone()
    for graphed in (True, False):
        ev = _evaluator(tr.model, graphed=graphed)
        for _ in range(2):                                    # the capture, then a replay
            ev.evaluate()
            assert tr.model.training
            assert all(u is v for u, v in zip(_usage(tr.model), usage)) and all(torch.equal(u, s) for u, s in zip(usage, saved))
            assert dict(ops._seed_state) == seed_state and torch.equal(ops.step_counter(DEV), ctr)
    tr.model.eval()
    _evaluator(tr.model, graphed=False).evaluate()
    assert not tr.model.training
    assert all(torch.equal(p, q) for p, q in zip(tr.model.parameters(), params))
    for p, g in zip(tr.model.parameters(), grads):
        assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))


def _full_state(tr):
    """Everything the next training step reads or continues from, as (name, clone) pairs: parameters, gradient buffers, optimizer moments
    and step counts, EMA profiles and their step, the routed-row counters, the device step counter of the seed stream, the generator's
    static buffers, the static text buffer and the captured step's loss -- plus the host side (seed stream, learning rates, mode)."""
    from hdmoe_hip import ops
    st = [(f"p.{n}", p) for n, p in tr.model.named_parameters()]
    st += [(f"g.{n}", p.grad) for n, p in tr.model.named_parameters() if p.grad is not None]
    st += [(f"opt.{i}.{k}", v) for i, s in tr.optimizer.state_dict()["state"].items() for k, v in s.items() if torch.is_tensor(v)]
    st += [(f"ema{k}.{n}", v) for k in range(tr.ema.nprofiles) for n, v in tr.ema.profile_state_dict(k).items()]
    st += [("ema.step", tr.ema._step), ("seed.ctr", ops.step_counter(DEV))]
    st += [(f"usage.{i}", u) for i, u in enumerate(_usage(tr.model))]
    st += [(f"in.{k}", v) for k, v in tr.inputs.data_buf.items()] + [("text", tr._text), ("loss", tr._staged.out["loss"]["loss"])]
    host = (dict(ops._seed_state), [g["lr"] for g in tr.optimizer.param_groups], tr.model.training, tr.step_idx)
    return [(n, t.detach().clone()) for n, t in st], host


def test_evaluation_is_invisible_to_a_graphed_trainer(tmp_path, capsys):
    """A graphed trainer with evaluator=..., eval_every=1 and an EMA (raw weights and both profiles evaluated behind every update), three
    steps, beside a trainer without an evaluator.

    Two free-running trainers cannot be compared bit for bit here, with or without an evaluator: the backward's fp32 atomics make a
    training step differ in the last bits from run to run (measured on an MI355X, two identical graphed trainers WITHOUT an evaluator:
    20 of 294 parameter tensors differ after one step, 168 after three, worst relative difference 6.8e-6; with an evaluator against
    without, 148 of 294 and 4.3e-6 -- the same noise).  What an invisible evaluation means is therefore asserted where it is exact:
      * around EVERY evaluate() call of the run the whole training state (`_full_state`) is bit-identical before and after;
      * the plain trainer starts every step from the evaluated trainer's weights (test_latent_dataset.py's lockstep) and the two losses
        -- the forward is deterministic -- are bit-identical in every step: the captured step still reads what training left.
    Also the wiring: last_eval, and one <run>_validation.jsonl record per evaluation and tag."""
    import hdmoe_hip
    from graphs.logger import Logger
    from hdmoe_hip import bank
    from hdmoe_hip.ema import WeightEMA
    hdmoe_hip.manual_seed(99)
    model = _model(train=True)
    ema = WeightEMA(model)
    ev = _evaluator(model, ema=ema, rounds=1)
    A = _tiny_trainer(model, dataset=_dataset(), batch_size=B, seed=TSEED, graphed=True, ema=ema, evaluator=ev, eval_every=1,
                      logger=Logger(log_dir=str(tmp_path), run_name="run"))
    plain_model = _model(train=True)
    P = _tiny_trainer(plain_model, dataset=_dataset(), batch_size=B, seed=TSEED, graphed=True, ema=WeightEMA(plain_model))
    assert A.last_eval is None and P.evaluator is None and P.eval_every is None
    inner, calls = ev.evaluate, []

    def checked(**kw):
        before, host = _full_state(A)
        res = inner(**kw)
        after, host2 = _full_state(A)
        assert host == host2, kw
        assert [n for n, _ in before] == [n for n, _ in after]
        bad = [n for (n, u), (_, v) in zip(before, after) if not torch.equal(u, v)]
        assert not bad, (kw, bad[:5], len(bad))
        calls.append((kw, len(before)))
        return res

    ev.evaluate = checked
    for step in range(3):
        P.model.load_state_dict(A.model.state_dict())
        bank.note_weights_changed()
        la = A.train_step()["loss"]["loss"].detach().clone()                 # read behind the three evaluations of the step
        lp = P.train_step()["loss"]["loss"].detach().clone()
        print(f"step {step}: loss with evaluator {float(la):.9g}, without {float(lp):.9g}")
        assert torch.equal(la, lp), step
        assert A.last_eval["step"] == step + 1 and set(A.last_eval["results"]) == {"raw", "ema0", "ema1"}
        assert A.last_eval["results"]["raw"]["n"] == N and A.model.training and P.last_eval is None
    capsys.readouterr()
    assert [kw for kw, _ in calls] == [{}, {"profile": 0}, {"profile": 1}] * 3 and all(n > 1000 for _, n in calls)
    recs = [json.loads(line) for line in (tmp_path / "run_validation.jsonl").read_text().splitlines()]
    assert [(r["step"], r["tag"]) for r in recs] == [(s, t) for s in (1, 2, 3) for t in ("raw", "ema0", "ema1")]
    last = A.last_eval["results"]
    assert recs[-3]["mse"] == last["raw"]["mse"].tolist() and recs[-1]["mse"] == last["ema1"]["mse"].tolist()
    assert last["raw"]["mse"].tolist() != last["ema0"]["mse"].tolist()


def test_eval_every_two_on_an_eager_trainer():
    model = _model(train=True)
    tr = _tiny_trainer(model, dataset=_dataset(), batch_size=B, seed=TSEED, evaluator=_evaluator(model, rounds=1, graphed=False), eval_every=2)
    seen = []
    for step in range(4):
        tr.train_step()
        seen.append(None if tr.last_eval is None else tr.last_eval["step"])
    assert seen == [None, 2, 2, 4] and set(tr.last_eval["results"]) == {"raw"}
