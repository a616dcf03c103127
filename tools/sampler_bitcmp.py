"""Bit comparison of Utils/EDM_sampler.py (and the model passes behind it) between two trees of the Python sources, on ONE compiled library:
    python tools/sampler_bitcmp.py PARENT_TREE [NEW_TREE]          (NEW defaults to this tree; PARENT PARENT checks reproducibility)
A tree is a directory that holds heterogeneous-moe-for-diffusion-models_amd/ and include/ (for the parent: `git archive <commit>` of the
two, unpacked somewhere outside the repository's history); the library is this tree's libhdmoe_hip.so for both (HDMOE_LIB_PATH).  Each
tree runs in its own process, one after the other, on the model of tests/golden/full_config2.pt at B = 2, latents (2, 4, R, R), N = 4
steps (tiled cases: (2, 4, R, R + R/2), tile (R, R), overlap R/2, T = 2).  For every configuration of CONFIGS the worker seeds torch and
the library's stream, builds one sampler and calls sample() (or denoise()) twice with different seeded noise, text, masks and scales of
the same shapes (five configurations at the end of the sample() list give the second call one more operand instead: four must
recapture, one must not; the worker asserts every flag), and writes one line: the SHA-256 of both results (for denoise() with a
momentum buffer, of the buffer too), whether the second call recaptured (another stage / evaluation state than after the first), and -- eager configurations -- the SHA-256 of the sequence of
entry-point names in _lib.CALL_LOG during the second call.
The list covers: the three solvers fused (fp32) and on the host loops (bf16 latents), eager and use_graph; host churn and churn_on_device;
guidance 1 and a float scale, two-pass and shared; a per-sample vector; an interval with a boundary inside the run on Heun and 2M; rescale
alone; APG with momentum on the fused path and on the captured "eval" state; composed K = 2 with masks, K = 3 without and the empty K = 1
case, two-pass and shared; init_latents with strength 0.5 and a soft inpaint_mask; both router masks; tiling with one chunk and with
tile_batch = half, with and without use_graph; one denoise() per guidance mode.
Prints both lists and the verdict; exit status 1 on any difference, 2 when a run did not finish."""
import hashlib, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "heterogeneous-moe-for-diffusion-models_amd"

APG = dict(apg_eta=0.5, apg_norm_threshold=5.0, apg_momentum=-0.5)
IV = dict(guidance_interval=(0.3, 20.0))          # N = 4: t = 80, ~9.7, ~0.47, 0.002 -- the first and the last stage lie outside
BF, GR, SH = dict(dtype="bf16"), dict(use_graph=True), dict(shared_guidance=True)
# (name, EDM_Sampler keywords beyond num_solve_steps=4 [guidance defaults to 2.0], features of the call)
CONFIGS = [(f"{sol} {'bf16 host' if bf else 'fp32 fused'} {'graph' if gr else 'eager'}",
            dict(solver=sol, **(BF if bf else {}), **(GR if gr else {})), {"seed"} if sol.endswith("sde") else set())
           for sol in ("heun", "dpmpp_2m", "dpmpp_2m_sde") for bf in (False, True) for gr in (False, True)] + [
    ("heun host churn eager", dict(S_churn=10.0), {"seed"}),
    ("heun host churn graph, library seed stream", dict(S_churn=10.0, **GR), set()),
    ("heun churn_on_device eager, library seed stream", dict(S_churn=10.0, churn_on_device=True), set()),
    ("heun churn_on_device graph", dict(S_churn=10.0, churn_on_device=True, **GR), {"seed"}),
    ("guidance 1 eager", dict(guidance=1.0), set()),
    ("guidance 1 graph, no uncond", dict(guidance=1.0, **GR), {"nounc"}),
    ("two-pass, no uncond, eager", {}, {"nounc"}),
    ("shared heun eager", SH, set()),
    ("shared heun graph", dict(**SH, **GR), set()),
    ("shared 2m bf16 graph", dict(solver="dpmpp_2m", **SH, **BF, **GR), set()),
    ("vector two-pass graph", GR, {"gvec"}),
    ("vector shared eager", SH, {"gvec"}),
    ("vector shared 2m bf16 eager", dict(solver="dpmpp_2m", **SH, **BF), {"gvec"}),
    ("interval heun graph", dict(**IV, **GR), set()),
    ("interval 2m eager", dict(solver="dpmpp_2m", **IV), set()),
    ("interval heun bf16 graph (eval variants)", dict(**IV, **BF, **GR), set()),
    ("interval 2m shared graph", dict(solver="dpmpp_2m", **IV, **SH, **GR), set()),
    ("rescale two-pass graph", dict(guidance_rescale=0.7, **GR), set()),
    ("rescale shared eager", dict(guidance_rescale=0.7, **SH), set()),
    ("apg momentum fused two-pass eager", APG, set()),
    ("apg momentum fused shared graph", dict(**APG, **SH, **GR), set()),
    ("apg momentum bf16 two-pass graph (eval state)", dict(**APG, **BF, **GR), set()),
    ("apg momentum bf16 shared eager", dict(**APG, **SH, **BF), set()),
    ("apg momentum interval vector 2m graph", dict(solver="dpmpp_2m", **APG, **IV, **GR), {"gvec"}),
    ("compose K=2 masks two-pass eager", {}, {"comp2m"}),
    ("compose K=2 masks shared graph", dict(**SH, **GR), {"comp2m"}),
    ("compose K=3 two-pass graph", GR, {"comp3"}),
    ("compose K=3 shared eager", SH, {"comp3"}),
    ("compose K=1 empty two-pass eager", {}, {"comp1"}),
    ("compose K=1 empty shared graph", dict(**SH, **GR), {"comp1"}),
    ("compose K=2 masks interval apg two-pass eager", dict(**IV, **APG), {"comp2m"}),
    ("compose K=3 interval apg shared bf16 graph", dict(**IV, **APG, **SH, **BF, **GR), {"comp3"}),
    ("img2img inpaint heun graph", GR, {"i2i"}),
    ("img2img inpaint heun bf16 eager", BF, {"i2i"}),
    ("img2img inpaint 2m bf16 graph", dict(solver="dpmpp_2m", **BF, **GR), {"i2i"}),
    ("img2img inpaint 2m sde eager", dict(solver="dpmpp_2m_sde"), {"i2i", "seed"}),
    ("router masks two-pass eager", {}, {"rmask"}),
    ("router masks shared graph", dict(**SH, **GR), {"rmask"}),
    ("tile one chunk eager", {}, {"tile"}),
    ("tile one chunk graph", GR, {"tile"}),
    ("tile half eager, vector, router masks", {}, {"tile", "half", "gvec", "rmask"}),
    ("tile half shared graph", dict(**SH, **GR), {"tile", "half"}),
    ("tile half 2m bf16 eager, img2img inpaint", dict(solver="dpmpp_2m", **BF), {"tile", "half", "i2i"}),
    ("tile half heun bf16 interval graph", dict(**IV, **BF, **GR), {"tile", "half"}),
    ("second call adds router masks, graph", GR, {"rmask@1"}),                                      # these recapture ...
    ("second call composes K=2 with masks, shared graph", dict(**SH, **GR), {"comp2m@1"}),
    ("second call is per-sample scales, eager", {}, {"gvec@1"}),
    ("second call inpaints, fused graph", GR, {"i2i@1"}),
    ("second call inpaints, bf16 graph (eval state)", dict(**BF, **GR), {"i2i@1"}),                 # ... this one must not
    ("denoise guidance 1", dict(guidance=1.0), {"denoise"}),
    ("denoise two-pass", {}, {"denoise"}),
    ("denoise two-pass guided=False", {}, {"denoise", "unguided"}),
    ("denoise shared", SH, {"denoise"}),
    ("denoise vector two-pass, router masks", {}, {"denoise", "gvec", "rmask"}),
    ("denoise vector shared", SH, {"denoise", "gvec"}),
    ("denoise rescale two-pass", dict(guidance_rescale=0.7), {"denoise"}),
    ("denoise apg momentum two-pass", APG, {"denoise", "mom"}),
    ("denoise apg momentum shared", dict(**APG, **SH), {"denoise", "mom"}),
    ("denoise compose K=2 masks two-pass", {}, {"denoise", "comp2m"}),
    ("denoise compose K=3 apg momentum shared", dict(**APG, **SH), {"denoise", "comp3", "mom"}),
    ("denoise compose K=2 masks shared guided=False", SH, {"denoise", "comp2m", "unguided"}),
]
TP, SOFT = -1.2, 1.6


def worker(tree, path):
    sys.path[:0] = [os.path.join(tree, PKG), os.path.join(tree, PKG, "Utils")]
    import torch
    from EDM_sampler import EDM_Sampler
    from hdmoe_hip import _lib, ops
    from models import model_config2
    dev = "cuda"
    g = torch.load(os.path.join(ROOT, "tests", "golden", "full_config2.pt"), weights_only=False)
    model = model_config2.preconditioned_HDMOEM(**g["cfg"])
    model.load_state_dict(g["state"])
    model = model.to(dev).eval()
    R, E, tshape = g["cfg"]["IN_img_resolution"], g["cfg"]["num_experts"], tuple(g["text"][:2].shape)

    def sha(*ts):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in ts:
            h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()[:16]

    def operands(feats, gen, j):
        """(positional arguments after the latents, keywords) of call j of a configuration: seeded values, the same shapes for both j"""
        rnd = lambda *shape: torch.randn(*shape, generator=gen)
        feats = {f[:-2] if f.endswith("@1") else f for f in feats if j == 1 or not f.endswith("@1")}      # "name@1": on the second call only
        W = R + R // 2 if "tile" in feats else R
        x, text, unc = rnd(2, 4, R, W).to(dev), rnd(*tshape).to(dev), rnd(*tshape).to(dev)
        kw = {}
        if "gvec" in feats:
            kw["guidance"] = torch.tensor([1.5, 3.0]) + 0.5 * torch.rand(2, generator=gen)
        if "comp2m" in feats:
            kw.update(compose_text=rnd(1, *tshape).to(dev), compose_weights=torch.rand(2, 2, generator=gen),
                      compose_masks=torch.rand(2, 2, R, R, generator=gen))
        if "comp3" in feats:
            kw.update(compose_text=rnd(2, *tshape).to(dev), compose_weights=rnd(3))
        if "comp1" in feats:
            kw.update(compose_text=torch.empty((0,) + tshape, device=dev))
        if "rmask" in feats:                                   # one expert closed per row (U-Net), one for the batch (ViT); they move with j
            um, vm = torch.ones(2, E), torch.ones(E)
            um[0, j % E], um[1, (j + 1) % E], vm[(j + 2) % E] = 0.0, 0.0, 0.0
            kw.update(Unet_router_mask=um, Vit_router_mask=vm.to(dev))
        if "denoise" in feats:
            kw["guided"] = "unguided" not in feats
            if "mom" in feats:
                kw["momentum_state"] = (0.1 * rnd(2, 4, R, W)).to(dev).contiguous()
            return (1.3 * x, torch.tensor(1.3, device=dev), text, TP, SOFT, None if "nounc" in feats else unc), kw
        if "i2i" in feats:
            kw.update(init_latents=rnd(2, 4, R, W).to(dev), strength=0.5, inpaint_mask=torch.rand(2, 1, R, W, generator=gen).to(dev))
        if "seed" in feats:
            kw["seed"] = 11 + j
        if "tile" in feats:
            kw.update(tile=(R, R), tile_overlap=R // 2, tile_batch=2 if "half" in feats else None)
        return (x, text, TP, SOFT, None if "nounc" in feats else unc), kw

    lines = []
    with torch.no_grad():
        for n, (name, ctor, feats) in enumerate(CONFIGS):
            torch.manual_seed(1000 + n)
            ops.manual_seed(1000 + n)
            gen = torch.Generator().manual_seed(2000 + n)
            ctor = dict(dict(guidance=2.0), **ctor)
            if ctor.get("dtype") == "bf16":
                ctor["dtype"] = torch.bfloat16
            s = EDM_Sampler(model, model, num_solve_steps=4, **ctor)
            digests, states = [], []
            for j in range(2):
                args, kw = operands(feats, gen, j)
                log = j == 1 and not s.use_graph
                if log:
                    _lib.CALL_LOG = []
                out = (s.denoise if "denoise" in feats else s.sample)(*args, **kw)
                digests.append(sha(out, *([kw["momentum_state"]] if "momentum_state" in kw else [])))
                if log:
                    names, _lib.CALL_LOG = "\n".join(name_ for name_, _ in _lib.CALL_LOG), None
                states.append((s._stage, s._graph))
            recap = int(states[0][0] is not states[1][0] or states[0][1] is not states[1][1])
            # same shapes and operands: one capture serves both calls; the "@1" cases recapture, but for the "eval" state, which
            # holds no known region
            want = int(any(f.endswith("@1") for f in feats) and "eval state" not in name)
            assert recap == want, f"{name}: recaptured={recap}, expected {want}"
            seq = f" launches={hashlib.sha256(names.encode()).hexdigest()[:16]}" if not s.use_graph else ""
            lines.append(f"{name}: {digests[0]} {digests[1]} recaptured={recap}{seq}")
            print(lines[-1], file=sys.stderr, flush=True)             # progress; the lists go to stdout at the end
    open(path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit("usage: sampler_bitcmp.py PARENT_TREE [NEW_TREE]")
    if sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
        sys.exit(0)
    trees = [os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT]
    env = dict(os.environ, HDMOE_LIB_PATH=os.environ.get("HDMOE_LIB_PATH") or os.path.join(ROOT, PKG, "hdmoe_hip", "libhdmoe_hip.so"))
    res = []
    with tempfile.TemporaryDirectory() as d:
        for i, tree in enumerate(trees):
            out = os.path.join(d, str(i))
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, out], env=env).returncode
            if rc:
                print(f"the run of {tree} ended with status {rc}: nothing compared")
                sys.exit(2)
            res.append(open(out).read().splitlines())
    la, lb = res
    print(f"== sampler_bitcmp: parent {os.path.relpath(trees[0], ROOT)}  against  {os.path.relpath(trees[1], ROOT)}  (one library)")
    print(f"-- parent ({len(la)})"); print("\n".join(la))
    print(f"-- new ({len(lb)})"); print("\n".join(lb))
    diff = [(a, b) for a, b in zip(la, lb) if a != b]
    for a, b in diff:
        print(f"DIFF {a}   |   new: {b.split(': ', 1)[1]}")
    ok = not diff and len(la) == len(lb) == len(CONFIGS)
    print(f"ALL {len(la)} IDENTICAL" if ok else f"{len(diff)} DIFFERENCES")
    sys.exit(0 if ok else 1)
