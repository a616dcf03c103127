"""bench.py --dump-outputs: one float32 .npy per output of the timed step, within the size cap, the same sample positions in every run."""
import os

import numpy as np
import torch


def _outputs():
    g = torch.Generator().manual_seed(0)
    return {"loss": torch.tensor(4.25), "grad.a.weights": torch.randn(64, 32, 3, 3, generator=g),
            "grad.b.bias": torch.randn(7, generator=g), "grad.c": torch.randn(1, generator=g)}


def test_step_outputs_are_the_loss_and_every_parameter_gradient():
    import bench
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    m[1].bias.requires_grad_(False)
    loss = m(torch.ones(5, 3)).square().mean()
    loss.backward()
    out = bench.step_outputs({"loss": loss}, m)
    assert list(out) == ["loss", "grad.0.weight", "grad.0.bias", "grad.1.weight"]
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in out.values())
    assert torch.equal(out["grad.1.weight"], m[1].weight.grad)


def test_dump_below_the_cap_is_complete(tmp_path):
    import bench
    outs = _outputs()
    bench.dump_outputs(outs, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in outs)
    for n, t in outs.items():
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())


def test_dump_above_the_cap_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 20000)
    outs = _outputs()
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in outs)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 20000
    big = np.load(tmp_path / "a" / "grad.a.weights.npy")
    assert big.dtype == np.float32 and 0 < big.size < outs["grad.a.weights"].numel()
    assert np.isin(big, outs["grad.a.weights"].numpy().ravel()).all()
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
