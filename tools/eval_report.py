#!/usr/bin/env python
"""Print the held-out evaluation records of a run (`Logger.log_evaluation`: <run>_validation.jsonl) as text: per record the per-level
table (sigma, count, mse +- its standard error, the EDM-weighted error, nll, log-variance) and the two (E x K) routing maps -- the mean
gate probability of every expert at every noise level, the measured counterpart of the reference's plot_expert_specialization_advanced.

    python tools/eval_report.py training_logs/experiment_validation.jsonl [--step 5000] [--tag raw] [--selected] [--png out.png]

--step / --tag pick records (default: the last step, every tag); --selected prints the fraction of samples with a probability > 0 in
place of the mean probability; --png also draws the maps, when matplotlib is installed."""
import argparse
import json
import sys

SHADES = " .:-=+*#%@"


def fmt(v, spec):
    return format("nan" if v is None else format(v, spec), ">11")


def level_table(rec) -> str:
    lines = [" ".join(format(h, ">11") for h in ("level", "sigma", "count", "mse", "stderr", "edm_w", "nll", "log_var"))]
    for k, sg in enumerate(rec["sigma"]):
        cells = [format(k, ">11"), fmt(sg, ".4g"), fmt(rec["count"][k], ".0f")]
        cells += [fmt(rec[key][k], ".5g") for key in ("mse", "mse_stderr", "edm_weighted", "nll", "log_var")]
        lines.append(" ".join(cells))
    return "\n".join(lines)


def usage_map(rows, title: str) -> str:
    """rows: K lists of E values in [0, 1] (None: a level without samples) -> E lines of K cells, value and a shade."""
    K, E = len(rows), len(rows[0]) if rows else 0
    lines = [f"{title}  (rows: experts, columns: levels 0 .. {K - 1}, low sigma to high as the levels are ordered)"]
    for e in range(E):
        cells = []
        for k in range(K):
            v = rows[k][e]
            cells.append("  nan " if v is None else f"{v:5.2f}{SHADES[min(int(max(v, 0.0) * len(SHADES)), len(SHADES) - 1)]}")
        lines.append(f"  e{e} " + " ".join(cells))
    return "\n".join(lines)


def report(rec, selected: bool) -> str:
    kind = "selected" if selected else "usage"
    head = f"step {rec['step']}  tag {rec['tag']}  n {rec['n']:.0f}  mse_mean {fmt(rec['mse_mean'], '.6g').strip()}"
    what = "fraction of samples with p > 0" if selected else "mean gate probability"
    return "\n".join([head, level_table(rec), usage_map(rec[f"unet_{kind}"], f"U-Net router, {what}"),
                      usage_map(rec[f"vit_{kind}"], f"ViT router, {what}")])


def draw(recs, selected: bool, path: str) -> bool:
    try:
        import matplotlib
    except ImportError:
        return False
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    kind = "selected" if selected else "usage"
    fig, axes = plt.subplots(len(recs), 2, figsize=(10, 3 * len(recs)), squeeze=False)
    for row, rec in zip(axes, recs):
        for ax, tag in zip(row, ("unet", "vit")):
            grid = [[float("nan") if v is None else v for v in level] for level in rec[f"{tag}_{kind}"]]
            im = ax.imshow(list(zip(*grid)), aspect="auto", vmin=0.0, vmax=1.0, cmap="viridis")
            ax.set_title(f"{tag} {kind}, step {rec['step']} ({rec['tag']})")
            ax.set_xlabel("noise level")
            ax.set_ylabel("expert")
            fig.colorbar(im, ax=ax)
    fig.tight_layout()
    fig.savefig(path)
    return True


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("path")
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--selected", action="store_true")
    ap.add_argument("--png", default=None)
    args = ap.parse_args(argv)
    with open(args.path) as f:
        recs = [json.loads(line) for line in f if line.strip()]
    if not recs:
        print(f"{args.path}: no records", file=sys.stderr)
        return 1
    step = recs[-1]["step"] if args.step is None else args.step
    recs = [r for r in recs if r["step"] == step and (args.tag is None or r["tag"] == args.tag)]
    if not recs:
        print(f"{args.path}: no record of step {step}" + ("" if args.tag is None else f" with tag {args.tag}"), file=sys.stderr)
        return 1
    print("\n\n".join(report(r, args.selected) for r in recs))
    if args.png is not None and not draw(recs, args.selected, args.png):
        print("matplotlib is not installed: no figure written", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
