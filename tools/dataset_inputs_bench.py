#!/usr/bin/env python
"""What making a step's batch from the device-resident dataset costs (`DeviceInputs.generate_from` + `text_from`: hdmoe_dataset_inputs,
hdmoe_text_gather_dropout), against the same batch made the way the trainer allowed before it: `index_select` of mean / std on a slice
of a device permutation, `randn`, the flip by `torch.where` over `flip(-1)`, the scale, `copy_` into the static latent buffer,
`DeviceInputs.generate`, and for the text `index_select` + `drop_text`.  (The permutation itself -- one `randperm` per epoch -- is left
out of the torch side's timed window.)

B = 256, latents (4, 32, 32) fp32 with std, flip 0.5, scale 0.09, text rows (77, 768) fp32, cond_dropout 0.1; N = 2040 with one text row
per item, N = 65536 with a 1000-row text table behind a text_index (65536 rows of 77 x 768 fp32 would be 15.5 GB).

One process, the two sides alternating; each round is `--launches` consecutive steps between two device events with the device idle
before it, and a host clock around the enqueue of the same steps.  `device_us` is event time per step (launch gaps included: when the
host is the slower side it is the host's time), `host_us` the enqueue time per step.

    python tools/dataset_inputs_bench.py [--rounds 20] [--launches 50] [--out profiles/r12_dataset_inputs.json]

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


def device_inputs(seed, p):
    from Utils import configs
    from Utils.utils import DeviceInputs, MaskGenerator, ZetaScheduler
    mc, mcfg, zc = configs.mask_configs, configs.model_configs, configs.zeta_configs
    mk = lambda attr, rng: MaskGenerator(expert_attributes=mc[attr], p_mean=mc["p_mean"], p_std=mc["p_std"], total_steps=mcfg["total_steps"],
                                         min_active=mc["min_active"], step_size=mc["step_size"], max_bandwidth=mc["max_BW"], bandwidth=mc["BW"],
                                         strat_band=mc["strat_band"], noise_range=mc[rng])
    zs = ZetaScheduler(total_steps=zc["total_schedule_steps"], max_zeta=zc["max_zeta"], min_zeta=zc["min_zeta"], strategy=zc["strategy"],
                       warmup_ratio=zc["warmup_ratio"])
    return DeviceInputs(mcfg, mc, zc, mk("unet_attr", "unet_noise_range"), mk("vit_attr", "vit_noise_range"), zs, seed=seed, rank=0, cond_dropout=p)


def case(N, K, args):
    import torch
    from Utils.utils import LatentDataset
    dev = torch.device("cuda", 0)
    B, chw, row = args.batch, (4, 32, 32), (77, 768)
    g = torch.Generator(device=dev).manual_seed(1234)
    mean = 0.5 * torch.randn((N,) + chw, device=dev, generator=g)
    std = 0.1 + torch.rand((N,) + chw, device=dev, generator=g)
    text = torch.randn((K,) + row, device=dev, generator=g)
    tidx = None if K == N else torch.randint(0, K, (N,), device=dev, generator=g).to(torch.int32)
    ds = LatentDataset(mean, std, scale=args.scale, flip=args.flip, text=text, text_index=tidx)
    spe = N // B

    fused_di, fused_text = device_inputs(99, args.p), torch.empty((B,) + row, device=dev)

    def fused(step):
        fused_di.generate_from(ds, step, B)
        fused_di.text_from(ds, step, out=fused_text)

    torch_di, lat, torch_text = device_inputs(99, args.p), torch.empty((B,) + chw, device=dev), torch.empty((B,) + row, device=dev)
    perm = torch.randperm(N, device=dev, generator=g)
    tlong = None if tidx is None else tidx.long()

    def by_torch(step):
        pos = step % spe
        idx = perm[pos * B:(pos + 1) * B]
        x0 = mean.index_select(0, idx) + std.index_select(0, idx) * torch.randn((B,) + chw, device=dev, generator=g)
        fl = torch.rand(B, device=dev, generator=g) < args.flip
        x0 = torch.where(fl.view(B, 1, 1, 1), x0.flip(-1), x0) * args.scale
        lat.copy_(x0)
        torch_di.generate(lat, step)
        rows = text.index_select(0, idx if tlong is None else tlong.index_select(0, idx))
        torch_di.drop_text(rows, step, out=torch_text)

    def timed(fn, first):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(args.launches):
            fn(first + i)
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.launches, 1e6 * (t1 - t0) / args.launches

    for fn in (fused, by_torch):                              # code objects loaded, buffers allocated, clocks up
        timed(fn, 0)
    dev_us, host_us = {"fused": [], "torch": []}, {"fused": [], "torch": []}
    for r in range(args.rounds):
        for name, fn in (("fused", fused), ("torch", by_torch)):
            d, h = timed(fn, r * args.launches)
            dev_us[name].append(d)
            host_us[name].append(h)
    res = dict(N=N, text_rows=K, text_index=tidx is not None, batch=B, latent=list(chw), text_row=list(row), dtype="float32", flip=args.flip,
               scale=args.scale, cond_dropout=args.p, launches_per_round=args.launches, rounds=args.rounds)
    for name in ("fused", "torch"):
        res[name] = dict(device_us=summary(dev_us[name]), host_us=summary(host_us[name]))
    for kind in ("device_us", "host_us"):
        f, t = res["fused"][kind], res["torch"][kind]
        res[kind + "_ranges_apart"] = f["max_us"] < t["min_us"] or t["max_us"] < f["min_us"]
        res[kind + "_torch_over_fused"] = round(t["median_us"] / f["median_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--flip", type=float, default=0.5)
    ap.add_argument("--scale", type=float, default=0.09)
    ap.add_argument("--sizes", default="2040:2040,65536:1000", help="N:K pairs, K == N: one text row per item, else a text_index")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_dataset_inputs.json"))
    args = ap.parse_args()
    res = {"note": "tools/dataset_inputs_bench.py on one MI355X, one process: the fused dataset calls against the torch ops + generate + drop_text "
                   "they replace, alternating rounds; device_us is event time per step with launch gaps, host_us the enqueue time per step."}
    for pair in args.sizes.split(","):
        N, K = (int(v) for v in pair.split(":"))
        res[f"N{N}"] = case(N, K, args)
        print(f"[dataset_inputs_bench] N={N}: fused {res[f'N{N}']['fused']['device_us']['median_us']} us device / "
              f"{res[f'N{N}']['fused']['host_us']['median_us']} us host, torch {res[f'N{N}']['torch']['device_us']['median_us']} / "
              f"{res[f'N{N}']['torch']['host_us']['median_us']}", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
