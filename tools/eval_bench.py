#!/usr/bin/env python
"""What the held-out evaluation costs per batch (csrc/evalstats.hip; Utils/evaluation.py), at BASELINE configs[1] shapes: B = 256,
latents (4, 32, 32) fp32, E = 4 experts, K = 16 levels.

  (a) the three new launches of a batch: `ops.eval_inputs` (one launch) and `ops.eval_accumulate` (two);
  (b) the same statistics composed from torch ops on the same tensors (per-sample mean of squares, the EDM weight, the clamped log-variance
      term, a one-hot (B, K) matrix and one fp64 matmul into the (K, 6 + 4E) table) -- what `eval_accumulate` replaces;
  (c) one graphed evaluation batch end to end (the eager input launches + the replay of forward + accumulate) with the bench model
      (model_config1, bf16), beside the replay of the same forward alone.

One process, the sides of a comparison alternating; each round is `--launches` consecutive batches between two device events with the
device idle before it, and a host clock around the enqueue of the same batches.  `device_us` is event time per batch (launch gaps
included: where the host is the slower side it is the host's time), `host_us` the enqueue time per batch.

    python tools/eval_bench.py [--rounds 20] [--launches 50] [--out profiles/r13_evaluator.json]

A difference counts where the two sides' ranges (min .. max over the rounds) are apart."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2), spread_us=round(max(us) - min(us), 2),
                rounds_us=[round(v, 2) for v in us])


def timed(fn, launches):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches, 1e6 * (t1 - t0) / launches


def compare(sides, args):
    """{name: {device_us, host_us}} for the callables of `sides`, alternating over the rounds, after one warm-up window each."""
    for fn in sides.values():
        timed(fn, args.launches)
    dev_us, host_us = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            d, h = timed(fn, args.launches)
            dev_us[name].append(d)
            host_us[name].append(h)
    return {name: dict(device_us=summary(dev_us[name]), host_us=summary(host_us[name])) for name in sides}


def apart(res, a, b):
    out = {}
    for kind in ("device_us", "host_us"):
        x, y = res[a][kind], res[b][kind]
        out[kind + "_ranges_apart"] = x["max_us"] < y["min_us"] or y["max_us"] < x["min_us"]
        out[f"{kind}_{b}_over_{a}"] = round(y["median_us"] / x["median_us"], 2)
    return out


def kernels(args):
    import torch
    from hdmoe_hip import ops
    dev = torch.device("cuda", 0)
    B, chw, E, K, N, sd = args.batch, (4, 32, 32), 4, 16, 2048, 0.5
    L = chw[0] * chw[1] * chw[2]
    g = torch.Generator(device=dev).manual_seed(1234)
    f32 = dict(dtype=torch.float32, device=dev)
    mean = 0.5 * torch.randn((N,) + chw, device=dev, generator=g)
    levels = torch.exp(torch.linspace(-4.0, 3.0, K, **f32))
    x, x0, sigma = torch.zeros((B,) + chw, **f32), torch.zeros((B,) + chw, **f32), torch.zeros(B, 1, 1, 1, **f32)
    level, item = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    den = torch.randn((B,) + chw, device=dev, generator=g)
    lv = torch.randn(B, 1, 1, 1, device=dev, generator=g)
    pU, pV = torch.rand(B, E, device=dev, generator=g), torch.rand(B, E, device=dev, generator=g)
    acc = torch.zeros(K, 6 + 4 * E, dtype=torch.float64, device=dev)
    acc_t = torch.zeros_like(acc)
    ws = torch.zeros(ops.eval_ws_floats(B, L), **f32)
    nb = N // B

    def inputs(i):
        ops.eval_inputs(x, x0, sigma, level, item, mean, levels, 99, i % K, (i % nb) * B, B, scale=0.09)

    def accumulate(i):
        ops.eval_accumulate(acc, ws, den, x0, sigma, level, lv, pU, pV, sd)

    def by_torch(i):
        mse = (den - x0).square().flatten(1).mean(1).double()
        sg = sigma.view(B).double()
        l = lv.view(B).clamp(-10.0, 10.0).double()
        rows = torch.cat([torch.ones(B, 1, dtype=torch.float64, device=dev), mse[:, None], (mse * mse)[:, None],
                          ((sg * sg + sd * sd) / (sg * sd) ** 2 * mse)[:, None], (mse * torch.exp(-l) + l)[:, None], l[:, None],
                          pU.double(), (pU > 0).double(), pV.double(), (pV > 0).double()], dim=1)
        onehot = (level.view(B, 1) == torch.arange(K, device=dev).view(1, K)).double()
        acc_t.add_(onehot.t() @ rows)

    inputs(0)
    res = compare({"eval_inputs": inputs, "eval_accumulate": accumulate, "torch_statistics": by_torch}, args)
    torch.cuda.synchronize()
    res["statistics"] = apart(res, "eval_accumulate", "torch_statistics")
    res["eval_inputs"]["bytes_moved"] = B * L * 4 * 3                     # the mean rows in, x0 and x out
    res["shapes"] = dict(batch=B, latent=list(chw), experts=E, levels=K, items=N, table_dtype="float32")
    return res


def graphed_batch(args):
    """BASELINE configs[1]'s model (what bench.py times) behind an Evaluator; the same forward captured alone for comparison."""
    import torch
    import hdmoe_hip
    from hdmoe_hip import graph as hgraph
    from models import model_config1
    from Utils import configs as C
    from Utils.evaluation import Evaluator
    from Utils.utils import LatentDataset
    dev = torch.device("cuda", 0)
    bc = C.BASELINE_CONFIGS[2]
    kw = C.model_kwargs(**bc["over"])
    torch.manual_seed(1234)
    model = model_config1.preconditioned_HDMOEM(**kw)
    with torch.no_grad():                                    # as bench.py: zero-inits would make the experts' output identically 0
        for n, p in model.named_parameters():
            if n.endswith("out_gain"):
                p.fill_(0.5)
            elif n.endswith("alpha_txt"):
                p.fill_(0.3)
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    model = model.to(dev).eval()
    B, N, K = args.batch, 2048, 16
    g = torch.Generator(device=dev).manual_seed(1234)
    mean = 0.5 * torch.randn(N, 4, 32, 32, device=dev, generator=g)
    text = torch.randn(64, 77, kw["text_emb_dim"], device=dev, generator=g)
    tidx = torch.randint(0, 64, (N,), device=dev, generator=g).to(torch.int32)
    ds = LatentDataset(mean, None, scale=1.0, text=text, text_index=tidx)
    mcfg = dict(C.model_configs, **bc["over"])
    ev = Evaluator(model, mcfg, C.mask_configs, ds, B, levels=K, rounds=1, seed=99, graphed=True)
    t0 = time.perf_counter()
    first = ev.evaluate()                                    # captures
    t1 = time.perf_counter()
    again = ev.evaluate()
    t2 = time.perf_counter()
    batches = list(ev._batches())
    b = ev.buf

    def forward_only():
        with torch.no_grad():
            return model(x=b["x"], sigma=b["sigma"], text_emb=b["text"], Unet_router_mask=b["umask"], Vit_router_mask=b["vmask"], zeta=0.0,
                         **ev._model_extra)

    fwd = hgraph.GraphedStep(forward_only, dev)
    model._hdmoe_bank.refresh_eval()

    def batch(i):
        ev._inputs(*batches[i % len(batches)])
        ev._step()

    res = compare({"evaluation_batch": batch, "forward_replay_alone": lambda i: fwd()}, args)
    torch.cuda.synchronize()
    res["batch"] = apart(res, "forward_replay_alone", "evaluation_batch")
    res["whole_evaluation"] = dict(items=N, batches=len(batches), first_call_with_capture_s=round(t1 - t0, 3), second_call_s=round(t2 - t1, 4),
                                   same_bits=bool((first["acc"].view("int64") == again["acc"].view("int64")).all()),
                                   mse_mean=first["mse_mean"])
    res["model"] = "BASELINE configs[1]: model_config1 preconditioned_HDMOEM, bf16 compute, eval mode, B = %d" % B
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip (c), the graphed evaluation batch of the bench model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_evaluator.json"))
    args = ap.parse_args()
    res = {"note": "tools/eval_bench.py on one MI355X, one process, sides alternating; device_us is event time per batch with launch gaps, "
                   "host_us the enqueue time per batch.  Every figure in this file was measured by that run."}
    res["kernels"] = kernels(args)
    k = res["kernels"]
    print(f"[eval_bench] eval_inputs {k['eval_inputs']['device_us']['median_us']} us, eval_accumulate "
          f"{k['eval_accumulate']['device_us']['median_us']} us, torch statistics {k['torch_statistics']['device_us']['median_us']} us "
          f"(host {k['eval_accumulate']['host_us']['median_us']} / {k['torch_statistics']['host_us']['median_us']})", file=sys.stderr, flush=True)
    if not args.no_model:
        res["graphed_batch"] = graphed_batch(args)
        gb = res["graphed_batch"]
        print(f"[eval_bench] evaluation batch {gb['evaluation_batch']['device_us']['median_us']} us, forward replay alone "
              f"{gb['forward_replay_alone']['device_us']['median_us']} us", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
