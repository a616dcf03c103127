"""Dev tool: cost of the EDM_Sampler solvers at the BASELINE configs[4] per-GPU share (B = 128, 4x64x64 latents, 8 experts, bf16, hipGraph
replay of whole solver stages): Heun at N = 40 (2N - 1 evaluations) against DPM-Solver++(2M) at N = 40 and N = 20 (N evaluations), in one
process, each mode on its own sampler (its own capture), timed runs interleaved.  Prints one JSON line.
usage: sampler_solver_bench.py [--batch 128] [--steps 40] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils")]
import torch  # noqa: E402
import hdmoe_hip  # noqa: E402
from Utils import configs  # noqa: E402
from Utils.EDM_sampler import EDM_Sampler  # noqa: E402
from models import model_config2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("needs a GPU")
B, N = args.batch, args.steps
hdmoe_hip.set_compute_dtype(torch.bfloat16)
kw = configs.model_kwargs(**configs.BASELINE_CONFIGS[4]["over"])
torch.manual_seed(0)
model = model_config2.preconditioned_HDMOEM(**kw).cuda().eval()
with torch.no_grad():
    for n, p in model.named_parameters():
        if n.endswith("out_gain"):
            p.fill_(0.5)
gen = torch.Generator(device="cuda").manual_seed(0)
noise = torch.randn(B, 4, 64, 64, device="cuda", generator=gen)
text = torch.randn(B, 77, kw["text_emb_dim"], device="cuda", generator=gen)
modes = {f"heun_N{N}": ("heun", N), f"dpmpp_2m_N{N}": ("dpmpp_2m", N), f"dpmpp_2m_N{N // 2}": ("dpmpp_2m", N // 2)}
samplers = {k: EDM_Sampler(model, Guide_net=model, guidance=1.0, num_solve_steps=n, use_graph=True, solver=sv) for k, (sv, n) in modes.items()}
times = {k: [] for k in modes}
with torch.no_grad():
    for k, s in samplers.items():                                   # warm-up + capture
        out = s.sample(noise, text, -1.2, 1.2)
        assert torch.isfinite(out).all(), k
        assert s.fused_heun if modes[k][0] == "heun" else s.fused_dpm, k
    for _ in range(args.reps):
        for k, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.sample(noise, text, -1.2, 1.2)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
res = {}
for k, (sv, n) in modes.items():
    n_eval = 2 * n - 1 if sv == "heun" else n
    dt = statistics.median(times[k])
    res[k] = dict(evals=n_eval, s=round(dt, 4), imgs_per_s=round(B / dt, 1), ms_per_eval=round(1e3 * dt / n_eval, 3),
                  runs_s=[round(t, 4) for t in times[k]])
heun, dpm = res[f"heun_N{N}"], res[f"dpmpp_2m_N{N}"]
res["dpm_vs_heun_imgs_per_s"] = round(dpm["imgs_per_s"] / heun["imgs_per_s"], 3)
res["dpm_vs_heun_ms_per_eval"] = round(dpm["ms_per_eval"] / heun["ms_per_eval"], 4)
print(json.dumps(dict(metric="sampler_solver", B=B, N=N, reps=args.reps, **res)))
