"""Rebuild the EMA of another sigma_rel from saved snapshots and write it as a checkpoint, on one GPU.

    python tools/posthoc_ema.py --snapshots run/ema --checkpoint run/ckpt.pt --sigma-rel 0.075 --out run/ckpt_ema0075.pt [--step 20000]

--snapshots : a directory of WeightEMA.save_snapshot files (Trainer(..., ema_snapshot_every=, ema_snapshot_dir=) writes them); may be given
              several times, and may name single files or checkpoints that carry "ema_state_dict"
--checkpoint: a Utils.training.save_checkpoint file: its "config" builds the model, its buffers and every other key are kept
--out       : the same dictionary with "model_state_dict" holding the reconstructed average (and without optimizer / EMA state)
Prints the fit error (the relative part of the wanted profile the snapshots cannot represent).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", action="append", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--sigma-rel", type=float, required=True)
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--module", type=int, default=2, choices=(1, 2), help="models.model_config1 or model_config2")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("posthoc_ema needs a GPU: the combination runs on the device, there is no CPU path")
    from Utils import configs
    from hdmoe_hip import posthoc
    from models import model_config1, model_config2
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    cfg = ck["config"].get("model_configs", ck["config"])
    model = (model_config1 if args.module == 1 else model_config2).preconditioned_HDMOEM(**configs.model_kwargs(cfg))
    model.load_state_dict(ck["model_state_dict"])
    model = model.to("cuda")
    rec = posthoc.reconstruct(model, args.snapshots, sigma_rels=[args.sigma_rel], step=args.step)
    rec.copy_to(model, 0)
    out = {k: v for k, v in ck.items() if k not in ("optimizer_state_dict", "ema_state_dict")}
    out["model_state_dict"] = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    out["step"] = rec.step
    out["posthoc_ema"] = {"sigma_rel": args.sigma_rel, "gamma": rec.gammas[0], "step": rec.step, "fit_error": float(rec.fit_error[0]),
                          "sources": int(rec.weights.shape[0])}
    torch.save(out, args.out)
    print(f"sigma_rel {args.sigma_rel} at step {rec.step} from {rec.weights.shape[0]} saved profiles: fit_error {rec.fit_error[0]:.3e}, "
          f"max |weight| {abs(rec.weights).max():.3f} -> {args.out}")


if __name__ == "__main__":
    main()
