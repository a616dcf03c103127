"""Trainer(cond_dropout=p, null_text_emb=...): the text-conditioning dropout that trains the unconditional branch of classifier-free
guidance, in the trainer's three input modes (graphed replay, eager device inputs, torch's generator), its key (seed, rank, step), resume,
the checkpoint key and the error paths.  The keep decisions are judged by the numpy Philox of test_text_dropout.py (anchored to the library
there), copied here so that the file stands alone."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x0BADC0FFEE123457
GOLDEN = 0x9E3779B97F4A7C15


def keep_ref(seed, step, B, p):
    """1 - [d_i < float32(p)], d_i = u01(word i % 4 of Philox4x32-10 block (i / 4, 1)) under the key seed + (4 step + 3) golden."""
    key = (seed + (4 * step + 3) * GOLDEN) & ((1 << 64) - 1)
    n = (B + 3) // 4
    c = [np.arange(n, dtype=np.uint64), np.ones(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)]
    k0, k1, lo = key & 0xFFFFFFFF, key >> 32, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    w = np.stack(c, axis=1).astype(np.uint32).reshape(-1)[:B]
    d = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return (~(d < np.float32(p))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ models and configs
TINY = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
            VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8, top_k=2)


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model


def _tiny_trainer(device=DEV, **kw):
    """The small config-2 model of test_trainer_graphed.py's default-path test: zeta 0 and every dropout p = 0, so a step is a function
    of its weights and inputs alone."""
    from Utils import configs, training
    from models import model_config2
    mcfg = dict(configs.model_configs, **TINY, total_steps=10)
    zeta = dict(configs.zeta_configs, total_schedule_steps=4, max_zeta=0.0, min_zeta=0.0, warmup_ratio=0.0)
    torch.manual_seed(0)
    model = _no_dropout(model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg)).to(device).train())
    return training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, zeta, **kw)


def _tiny_batch(B=8, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return 0.5 * torch.randn(B, 4, 16, 16, device=DEV, generator=g), torch.randn(B, 5, 32, device=DEV, generator=g)


def _run(tr, lat, texts):
    """text_keep per step of len(texts) steps."""
    keeps = [tr.train_step(lat, text)["text_keep"].clone() for text in texts]
    torch.cuda.synchronize()
    return keeps


def _lockstep(A, B, lat, texts_a, texts_b):
    """A and B step side by side, B starting every step from A's weights and both from the same library seed.  The forward is
    deterministic, so what the two report for a step is comparable bit for bit; the backward adds weight gradients with fp32 atomics
    ("Determinism"), so the weights behind a step are not: two identical eager device-input trainers left to run freely
    differed after three steps in 93 - 97 of these 294 tensors by up to 2.4e-7, and in the third loss in two trials of three.
    Returns per step (A's result, B's result, A's and B's value of the library seed stream behind the step)."""
    import hdmoe_hip
    from hdmoe_hip import bank, ops
    out = []
    for ta, tb in zip(texts_a, texts_b):
        B.model.load_state_dict(A.model.state_dict())
        bank.note_weights_changed()
        step = []
        for tr, text in ((A, ta), (B, tb)):
            hdmoe_hip.manual_seed(99)
            res = tr.train_step(lat, text)
            step.append((dict(res, loss=res["loss"]["loss"].detach().clone()), ops.next_seed()))
        torch.cuda.synchronize()
        out.append((step[0][0], step[1][0], step[0][1], step[1][1]))
    return out


@pytest.fixture
def bf16():
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------------ p = 0 and p = 1
@gpu
def test_p0_changes_nothing(bf16, monkeypatch):
    """cond_dropout = 0.0 beside the keyword left out, three steps in lockstep: bit-equal losses, the same entry points in the same order
    (none of them the new one), the same state of torch's generator and of the library's seed stream, no new key.  The parameters behind
    the last step are held to 1e-6 of max(|a|, 1), four times the run-to-run spread of the unchanged trainer against itself (see _lockstep): bit
    equality of the weights is not a property of two runs of this training step."""
    from hdmoe_hip import ops
    lat, text = _tiny_batch()
    texts = [text, text.roll(1, 0), text.roll(2, 0)]
    names = []
    inner = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), inner(name, *a))[1])
    A = _tiny_trainer(cond_dropout=0.0, device_inputs=True, seed=SEED)
    B = _tiny_trainer(device_inputs=True, seed=SEED)
    torch.cuda.manual_seed(1234)
    state = torch.cuda.get_rng_state(DEV)
    for step, (ra, rb, sa, sb) in enumerate(_lockstep(A, B, lat, texts, texts)):
        print(f"step {step}: loss {float(ra['loss']):.9g} / {float(rb['loss']):.9g}")
        assert set(ra) == set(rb) == {"loss", "out_model", "sigma"}
        assert torch.equal(ra["loss"], rb["loss"]), step
        assert sa == sb
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    assert "hdmoe_train_inputs" in names and "hdmoe_text_dropout" not in names
    per_side = {}
    mark = [i for i, n in enumerate(names) if n == "hdmoe_train_inputs"]          # one per train_step: A, B, A, B, A, B
    assert len(mark) == 6
    for k, (lo, hi) in enumerate(zip(mark, mark[1:] + [len(names)])):
        per_side.setdefault(k % 2, []).append(names[lo:hi])
    assert per_side[0][1:] == per_side[1][1:] and len(per_side[0][1]) > 20      # (a first step also loads and registers, once per process)
    worst = max(float(((a - b).abs() / a.abs().clamp(min=1.0)).max()) for a, b in zip(A.model.parameters(), B.model.parameters()))
    print(f"parameters behind the last step: max |a - b| / max(|a|, 1) = {worst:.3e}")
    assert worst <= 1e-6
    assert A.inputs.keep is None and A.inputs.text is None


@gpu
def test_p1_is_training_on_the_null_text(bf16):
    """cond_dropout = 1.0 fed real text beside cond_dropout = 0.0 fed null_text(null, text), two steps in lockstep: the same kernels
    see the same bits, so the losses are bit-equal; text_keep is all zero."""
    from Utils.utils import null_text
    lat, text = _tiny_batch()
    texts = [text, text.roll(1, 0)]
    null = torch.randn(5, 32, generator=torch.Generator().manual_seed(3))
    fed = null_text(null, text)
    assert fed.shape == text.shape and fed.dtype == text.dtype and fed.device == text.device
    assert torch.equal(fed, null.to(DEV).expand_as(text))
    assert torch.equal(null_text(None, text), torch.zeros_like(text))
    A = _tiny_trainer(cond_dropout=1.0, null_text_emb=null, device_inputs=True, seed=SEED)
    B = _tiny_trainer(cond_dropout=0.0, device_inputs=True, seed=SEED)
    C = _tiny_trainer(device_inputs=True, seed=SEED)
    for step, (ra, rb, _, _) in enumerate(_lockstep(A, B, lat, texts, [fed, fed])):
        print(f"step {step}: loss {float(ra['loss']):.9g} / {float(rb['loss']):.9g}")
        assert torch.equal(ra["text_keep"], torch.zeros(8, device=DEV)) and "text_keep" not in rb
        assert torch.equal(ra["loss"], rb["loss"]), step
        if step == 0:                                           # and the text does matter to this model
            rc = C.train_step(lat, text)
            assert not torch.equal(rc["loss"]["loss"].detach(), ra["loss"])


# ------------------------------------------------------------------------------------------------------------------ eager vs graphed
def _wide_model():
    """BASELINE config 2 at its real width with the recipe's weights, no dropout: test_trainer_graphed.py's _model(2)."""
    from Utils import configs
    from models import model_config2
    from oracle.recipe import fill_state
    model = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(**configs.BASELINE_CONFIGS[2]["over"]))
    model.load_state_dict(fill_state(model.state_dict(), 5))
    return _no_dropout(model.to(DEV).train())


def _wide_trainer(**kw):
    from Utils import configs, training
    mcfg = dict(configs.model_configs, top_k=2, total_steps=4)
    mask = dict(configs.mask_configs, step_size=0.5)
    zeta = dict(configs.zeta_configs, total_schedule_steps=4, max_zeta=0.0, min_zeta=0.0, warmup_ratio=0.0)
    return training.Trainer(_wide_model(), mcfg, configs.optim_configs, configs.loss_configs, mask, zeta, **kw)


def _follow(dst, src):
    from hdmoe_hip import bank
    dst.model.load_state_dict(src.model.state_dict())
    bank.note_weights_changed()


@gpu
def test_graphed_and_eager_drop_the_same_samples(bf16):
    """p = 0.5, B = 8, three steps whose texts differ: both modes report the reference's keep under (seed, rank 0, step), their losses
    agree to test_trainer_graphed.py's bf16 bound (1e-3 relative; the eager side starts every step from the graphed side's weights and
    has run twice before, as there), and after each replay the static text buffer holds that step's text or the null row."""
    from oracle.recipe import make_inputs
    B, p = 8, 0.5
    inp = make_inputs(B, 4, 32, 4, 77, 768, 5)
    lat, text = inp["x0"].to(DEV), inp["text"].to(DEV)
    texts = [text, text.roll(1, 0) * 0.5, text.flip(0) + 0.25]
    null = torch.randn(77, 768, generator=torch.Generator().manual_seed(3)).to(DEV)
    G = _wide_trainer(graphed=True, seed=SEED, cond_dropout=p, null_text_emb=null)
    E = _wide_trainer(device_inputs=True, seed=SEED, cond_dropout=p, null_text_emb=null)
    for _ in range(2):
        E.train_step(lat, text)
    E.step_idx = 0
    inner = G._build_staged

    def build(*a, **k):                                         # the capture's warm-up runs renormalise G's weights: E copies them after it
        inner(*a, **k)
        _follow(E, G)

    G._build_staged = build
    seen = []
    for step in range(3):
        _follow(E, G)
        rg = G.train_step(lat, texts[step])
        lg, kg = rg["loss"]["loss"].detach().clone(), rg["text_keep"].clone()
        buf = G._text.clone()
        re_ = E.train_step(lat, texts[step])
        torch.cuda.synchronize()
        le, ke = re_["loss"]["loss"].detach(), re_["text_keep"]
        want = torch.from_numpy(keep_ref(SEED, step, B, p)).to(DEV)
        print(f"step {step}: loss graphed {float(lg):.7g} eager {float(le):.7g}, keep {kg.tolist()}")
        assert torch.equal(kg, want) and torch.equal(ke, want), (step, kg, ke, want)
        assert abs(float(lg) - float(le)) <= 1e-3 * abs(float(le)) + 1e-6
        rows = torch.where(want.bool().view(B, 1, 1), texts[step], null.expand_as(text))
        assert torch.equal(buf, rows), step
        assert torch.equal(E.inputs.text, rows), step
        seen.append(kg)
    assert 0 < float(seen[0].sum()) < B and not torch.equal(seen[0], seen[1])
    assert G.inputs.text is None                                 # the graphed trainer wrote into its own static buffer, no second one


# ------------------------------------------------------------------------------------------------------------------ resume
@gpu
def test_resume_reproduces_a_steps_decision(bf16):
    lat, text = _tiny_batch()
    keeps = _run(_tiny_trainer(cond_dropout=0.5, device_inputs=True, seed=SEED), lat, [text, text])
    T = _tiny_trainer(cond_dropout=0.5, device_inputs=True, seed=SEED)
    T.step_idx = 1
    res = T.train_step(lat, text)
    assert T.step_idx == 2
    assert torch.equal(res["text_keep"], keeps[1]) and not torch.equal(keeps[0], keeps[1])
    assert torch.equal(keeps[1].cpu(), torch.from_numpy(keep_ref(SEED, 1, 8, 0.5)))


# ------------------------------------------------------------------------------------------------------------------ torch-generator mode
@gpu
def test_torch_generator_mode_substitutes_rows(bf16):
    B = 64
    lat, text = _tiny_batch(B)
    null = torch.randn(5, 32, generator=torch.Generator().manual_seed(3))
    tr = _tiny_trainer(cond_dropout=0.5, null_text_emb=null)
    assert not tr.device_inputs and tr.inputs is None
    fed, inner = [], tr.model.forward

    def forward(*a, **k):
        fed.append(k["text_emb"].clone())
        return inner(*a, **k)

    tr.model.forward = forward
    torch.cuda.manual_seed(1234)
    res = tr.train_step(lat, text)
    keep = res["text_keep"]
    torch.cuda.manual_seed(1234)
    assert torch.equal(keep, (torch.rand(B, device=DEV) >= 0.5).float())      # the first draw of the step, on torch's generator
    assert keep.shape == (B,) and keep.dtype == torch.float32 and 0 < float(keep.sum()) < B
    assert len(fed) == 1
    assert torch.equal(fed[0], torch.where(keep.bool().view(B, 1, 1), text, null.to(DEV).expand_as(text)))


# ------------------------------------------------------------------------------------------------------------------ checkpoint, errors
def test_checkpoint_carries_the_null_row_only_when_given(tmp_path):
    from Utils import configs, training
    from models import model_config2
    mcfg = dict(configs.model_configs, **TINY, save_dir=str(tmp_path))
    model = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg))
    opt = training.build_optimizer(model, configs.optim_configs)
    null = torch.randn(5, 32, generator=torch.Generator().manual_seed(3))
    path = training.save_checkpoint(model, opt, 7, 0.25, {"model_configs": mcfg}, "with_null.pt", null_text_emb=null)
    model2 = model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg))
    ck = training.load_checkpoint(path, model2, training.build_optimizer(model2, configs.optim_configs))
    assert set(ck) == {"step", "model_state_dict", "optimizer_state_dict", "mse", "config", "null_text_emb"}
    assert torch.equal(ck["null_text_emb"], null) and ck["null_text_emb"].device.type == "cpu"
    path = training.save_checkpoint(model, opt, 7, 0.25, {"model_configs": mcfg}, "without.pt")
    assert set(torch.load(path, weights_only=False)) == {"step", "model_state_dict", "optimizer_state_dict", "mse", "config"}


@gpu
def test_value_errors(bf16):
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _tiny_trainer(cond_dropout=bad)
        with pytest.raises(ValueError):
            _tiny_trainer(cond_dropout=bad, device_inputs=True, seed=1)
    with pytest.raises(ValueError):
        _tiny_trainer(cond_dropout=0.5, null_text_emb=[0.0] * 32)
    lat, text = _tiny_batch()
    wrong = torch.zeros(5, 16)
    for kw in (dict(), dict(device_inputs=True, seed=1)):       # the null row is checked against the first batch, in either input mode
        tr = _tiny_trainer(cond_dropout=0.5, null_text_emb=wrong, **kw)
        with pytest.raises(ValueError):
            tr.train_step(lat, text)
        assert tr.step_idx == 0
