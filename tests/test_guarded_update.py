"""FusedAdamW.step(clip=..., health=h) and WeightEMA.update(ok=h.ok): a good verdict is the unguarded update bit for bit, a bad one writes
nothing -- parameters, both moments, the per-tensor step counts, every EMA profile and the EMA step -- and clears the usage counters."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = (1, 3, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)
ODD_VIEW = 5003
MAX_NORM = 1.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()


class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


class Net(torch.nn.Module):
    """Two "experts" (the second one's tensors sit behind a usage flag that reads 0) and the rest, over the bag of sizes."""

    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        mk = lambda n, s: (s * torch.randn(n, generator=gen)).to(DEV)
        buf = torch.zeros(ODD_VIEW + 8, device=DEV)
        buf[1:1 + ODD_VIEW] = mk(ODD_VIEW, 0.5)
        self.experts = torch.nn.ModuleList([Bag([mk(SIZES[8], 1.0), mk(SIZES[0], 3.0), mk(SIZES[4], 0.1)]), Bag([mk(SIZES[5], 1.0)])])
        self.rest = Bag([mk(n, 10.0 ** (i - 2)) for i, n in enumerate((SIZES[1], SIZES[2], SIZES[3], SIZES[6], SIZES[7]))] + [buf[1:1 + ODD_VIEW]])
        assert self.rest.ps[-1].data_ptr() % 16 != 0


class Side:
    def __init__(self, seed=5, guarded=True):
        from hdmoe_hip.ema import WeightEMA
        from hdmoe_hip.optim import FusedAdamW, GradHealth
        self.net = Net(seed)
        self.params = list(self.net.parameters())
        self.opt = FusedAdamW([{"params": list(self.net.experts.parameters()), "lr": 1e-2},
                               {"params": list(self.net.rest.parameters()), "lr": 3e-3, "weight_decay": 0.1}])
        self.opt.track_expert_usage([self.net.experts])
        self.usage = torch.zeros(2, device=DEV)
        object.__setattr__(self.net.experts, "_hdmoe_usage", self.usage)
        self.ema = WeightEMA(self.net, sigma_rels=(0.05, 0.10))
        n_e0 = len(list(self.net.experts[0].parameters()))
        self.group_of = [0] * n_e0 + [1] + [2] * len(list(self.net.rest.parameters()))
        self.health = GradHealth(self.params, self.group_of, ["e0", "e1", "rest"]) if guarded else None
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.t = 0

    def step(self, grads, poison=None):
        """One update on `grads` (a list of host tensors); poison = (parameter index, element, value) planted in the gradient."""
        with torch.no_grad():
            for p, g in zip(self.params, grads):
                p.grad.copy_(g)
            if poison is not None:
                self.params[poison[0]].grad.view(-1)[poison[1]] = poison[2]
            self.usage.copy_(torch.tensor([2.0, 0.0]))
        if self.health is not None:
            self.health.measure(self.t)
            self.opt.step(clip=(self.params, MAX_NORM), health=self.health)
            self.ema.update(ok=self.health.ok)
        else:
            self.opt.step(clip=(self.params, MAX_NORM))
            self.ema.update()
        self.t += 1

    def state(self):
        """Every tensor the update may write, as integer views (byte comparison: NaN == NaN, -0 != +0)."""
        torch.cuda.synchronize()
        out = {}
        for i, p in enumerate(self.params):
            out[f"p{i}"] = p.detach().view(torch.int32).clone()
            for k in ("exp_avg", "exp_avg_sq", "step"):
                if k in self.opt.state[p]:
                    out[f"{k}{i}"] = self.opt.state[p][k].detach().reshape(-1).view(torch.int32).clone()
        for k, flat in enumerate(self.ema._flat):
            out[f"ema{k}"] = flat.view(torch.int32).clone()
        out["ema_step"] = self.ema._step.clone()
        return out


def grads_for(side, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(p.shape, generator=gen) for p in side.params]


def same(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_three_clean_steps_equal_the_unguarded_twin():
    A, B = Side(guarded=True), Side(guarded=False)
    for t in range(3):
        g = grads_for(A, 100 + t, scale=3.0 if t == 1 else 0.001)       # clipped and unclipped steps
        A.step(g)
        B.step(g)
        assert int(A.health.ok.item()) == 1
    sa, sb = A.state(), B.state()
    assert any(k.startswith("exp_avg_sq") for k in sa) and same(sa, sb) == []
    assert int(A.ema._step.item()) == 3
    e1 = A.params[3]                                                     # the unused expert's tensor: skipped by both, counters cleared
    assert float(A.opt.state[e1]["step"]) == 0.0 and float(A.usage.abs().sum()) == 0.0
    h = A.health.read()
    assert h["measured"] == 3 and h["skipped"] == 0 and h["last_skipped_step"] == -1 and h["ok"] == 1
    assert h["grad"]["numel"] == [sum(p.numel() for p, g in zip(A.params, A.group_of) if g == k) for k in range(3)]


@pytest.mark.parametrize("poison", [(0, 4096, float("nan")), (1, 0, float("inf")), (9, ODD_VIEW - 1, float("-inf"))], ids=["nan", "inf", "-inf"])
def test_a_poisoned_step_writes_nothing(poison):
    A = Side()
    A.step(grads_for(A, 1))
    before = A.state()
    A.step(grads_for(A, 2), poison=poison)
    after = A.state()
    assert same(before, after) == []
    assert int(A.health.ok.item()) == 0 and float(A.usage.abs().sum()) == 0.0
    h = A.health.read()
    assert (h["skipped"], h["skipped_in_a_row"], h["last_skipped_step"]) == (1, 1, 1)
    assert h["grad"]["nonfinite"] == [1 if g == A.group_of[poison[0]] else 0 for g in range(3)] and h["grad"]["total"]["nonfinite"] == 1


def test_clean_poisoned_clean_equals_clean_clean():
    A, B = Side(guarded=True), Side(guarded=False)
    g0, g1, g2 = grads_for(A, 10), grads_for(A, 11), grads_for(A, 12)
    A.step(g0); A.step(g1, poison=(0, 0, float("nan"))); A.step(g2)
    B.step(g0); B.step(g2)
    assert same(A.state(), B.state()) == []
    assert int(A.ema._step.item()) == 2


def test_the_overflow_verdict_skips_as_well():
    A = Side()
    A.step(grads_for(A, 1))
    before = A.state()
    g = grads_for(A, 2)
    g[0][5], g[7][2] = 1.5e19, 1.5e19                                    # finite elements, finite squares, a sum past fp32
    A.step(g)
    h = A.health.read()
    assert h["ok"] == 0 and h["grad"]["total"]["nonfinite"] == 0 and h["skipped"] == 1
    assert same(before, A.state()) == []


def test_a_health_over_another_parameter_list_is_refused():
    from hdmoe_hip.optim import GradHealth
    A = Side()
    A.step(grads_for(A, 1))
    before = A.state()
    other = GradHealth(list(reversed(A.params)), list(reversed(A.group_of)), ["e0", "e1", "rest"])
    other.measure(0)
    A.usage.copy_(torch.tensor([2.0, 0.0]))
    with pytest.raises(ValueError, match="another parameter list"):
        A.opt.step(clip=(A.params, MAX_NORM), health=other)
    with pytest.raises(ValueError, match="needs clip"):
        A.opt.step(health=A.health)
    assert same(before, A.state()) == [] and A.usage.tolist() == [2.0, 0.0]
