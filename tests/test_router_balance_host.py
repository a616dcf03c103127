"""Host side of the routers' selection bias (no kernel is launched): the Trainer's argument checks, the checkpoint dictionary with and
without the bias, the logger's record, and the world-2 sum of the routing counts (gloo, modelled on test_dp_gloo.py)."""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


BAD = [dict(balance_rate=0), dict(balance_rate=0.0), dict(balance_rate=-0.1), dict(balance_rate=True), dict(balance_rate="0.1"),
       dict(balance_rate=float("nan")), dict(balance_rate=float("inf")), dict(balance_rate=0.1, balance_bias_max=0),
       dict(balance_rate=0.1, balance_bias_max=-1.0), dict(balance_rate=0.1, balance_bias_max=None),
       dict(balance_rate=0.1, balance_bias_max=float("nan")), dict(balance_bias_max=False)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v!r}" for k, v in kw.items()) for kw in BAD])
def test_trainer_argument_errors_come_before_the_model_is_touched(kw):
    from Utils import configs, training
    with pytest.raises(ValueError, match="Trainer: balance_"):
        training.Trainer(_Untouchable(), configs.model_configs, configs.optim_configs, configs.loss_configs, configs.mask_configs,
                         configs.zeta_configs, **kw)


def test_router_balance_argument_errors():
    from hdmoe_hip.balance import RouterBalance
    import models.model_components as mc
    r = mc.Router(in_channels=4, time_dim=6, top_k=2, num_experts=5)
    for kw in (dict(rate=0.0), dict(rate=-1.0), dict(rate=True), dict(rate=0.1, bias_max=0.0), dict(rate=float("nan"))):
        with pytest.raises(ValueError, match="RouterBalance: "):
            RouterBalance(r, **kw)
    with pytest.raises(ValueError, match="no top-k router"):
        RouterBalance(torch.nn.Linear(2, 2), 0.1)
    assert "balance_bias" not in r._buffers                       # a refused construction enabled nothing


def _tiny_model(tmp_path):
    from Utils import configs
    from models import model_config2
    over = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
                VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8)
    mcfg = dict(configs.model_configs, **over, save_dir=str(tmp_path))
    return mcfg, model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg))


FIVE = {"step", "model_state_dict", "optimizer_state_dict", "mse", "config"}


def test_checkpoint_keys_with_and_without_the_bias(tmp_path):
    from hdmoe_hip.balance import RouterBalance
    from Utils import configs, training
    mcfg, model = _tiny_model(tmp_path)
    keys = list(model.state_dict())
    opt = training.build_optimizer(model, configs.optim_configs)
    bal = RouterBalance(model, 0.125, bias_max=0.5)
    assert [n for n, _ in bal.routers] == ["net.Unet_router", "net.vit_router"]
    assert list(model.state_dict()) == keys                       # non-persistent buffers: the reference's layout
    for i, (_, r) in enumerate(bal.routers):
        r.balance_bias.copy_(torch.arange(4, dtype=torch.float32) / 8 - 0.1875 + i)
    plain = torch.load(training.save_checkpoint(model, opt, 3, 0.5, {"model_configs": mcfg}, "plain.pt"), weights_only=False)
    assert set(plain) == FIVE
    path = training.save_checkpoint(model, opt, 3, 0.5, {"model_configs": mcfg}, "bal.pt", balance=bal)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == FIVE | {"router_balance"} and list(ck["model_state_dict"]) == keys
    assert ck["router_balance"]["rate"] == 0.125 and ck["router_balance"]["bias_max"] == 0.5

    _, model2 = _tiny_model(tmp_path)
    bal2 = RouterBalance(model2, 0.125, bias_max=0.5)
    addr = [r.balance_bias.data_ptr() for _, r in bal2.routers]
    training.load_checkpoint(path, model2, balance=bal2)
    for (_, a), (_, b) in zip(bal.routers, bal2.routers):
        assert torch.equal(a.balance_bias, b.balance_bias) and float(b.balance_bias.abs().sum()) > 0
    assert addr == [r.balance_bias.data_ptr() for _, r in bal2.routers]      # restored in place: a captured step keeps its pointer
    # a file without the key leaves the bias alone; a model without the feature loads a file with it
    training.load_checkpoint(os.path.join(str(tmp_path), "plain.pt"), model2, balance=bal2)
    assert torch.equal(bal.routers[0][1].balance_bias, bal2.routers[0][1].balance_bias)
    _, model3 = _tiny_model(tmp_path)
    training.load_checkpoint(path, model3)
    with pytest.raises(ValueError, match="RouterBalance.load_state_dict"):
        bal2.load_state_dict({"bias": {"net.Unet_router": torch.zeros(4)}})


def test_logger_writes_one_balance_record(tmp_path):
    from graphs.logger import Logger
    lg = Logger(log_dir=str(tmp_path), run_name="run", log_interval=1)
    lg.log_balance(7, {"net.Unet_router": {"bias": [0.125, -0.125], "load": [3, 1], "target": [2 << 20, 0]}})
    (rec,) = [json.loads(s) for s in (tmp_path / "run_balance.jsonl").read_text().splitlines()]
    assert rec == {"step": 7, "routers": {"net.Unet_router": {"bias": [0.125, -0.125], "load": [3, 1], "load_over_target": [1.5, None]}}}


# ---------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _TwoRouters(torch.nn.Module):
    def __init__(self):
        super().__init__()
        import models.model_components as mc
        self.Unet_router = mc.Router(in_channels=4, time_dim=6, top_k=2, num_experts=5)
        self.vit_router = mc.Router(in_channels=4, time_dim=6, top_k=2, num_experts=3)
        self.plain_router = mc.Router(in_channels=4, time_dim=6, top_k=1, num_experts=2)      # never enabled: not part of the exchange


def _counts(rank):
    """What each rank's forwards would have counted: (load, target) per enabled router, large enough to need 64 bits."""
    return {"Unet_router": ([3 + rank, 0, 7 * rank, 1, (1 << 40) + rank], [(5 + rank) << 20] * 5),
            "vit_router": ([rank, 2, 4], [(1 << 33) * (rank + 1), 11, 0])}


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hdmoe_hip import ops
    from hdmoe_hip.dp import GradBuckets
    ops.SIDE_STREAMS = True
    torch.manual_seed(0)
    model = _TwoRouters()
    model.Unet_router.enable_balance()
    model.vit_router.enable_balance()
    buckets = GradBuckets(model)
    assert len(buckets._balanced) == 2
    out = []
    for step in range(2):                                       # the second step: the exchange starts from what the update left (zeros)
        buckets.zero_grad()
        for name, (load, target) in _counts(rank).items():
            r = getattr(model, name)
            r.balance_load.copy_(torch.tensor(load) * (step + 1))
            r.balance_target.copy_(torch.tensor(target) * (step + 1))
        buckets.finish()
        out.append({name: (getattr(model, name).balance_load.tolist(), getattr(model, name).balance_target.tolist()) for name in _counts(rank)})
        assert getattr(model, "Unet_router").balance_load.dtype == torch.int64
    q.put((rank, out))
    dist.destroy_process_group()


def test_accumulators_are_summed_identically_on_both_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(got) == [0, 1] and got[0] == got[1]
    for step in range(2):
        for name in ("Unet_router", "vit_router"):
            want = tuple([(a + b) * (step + 1) for a, b in zip(_counts(0)[name][i], _counts(1)[name][i])] for i in (0, 1))
            assert tuple(got[0][step][name]) == want, (step, name)
