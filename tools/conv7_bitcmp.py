"""Bit comparison of the streaming conv kernels between two builds of the library ("Round 9"):
    python tools/conv7_bitcmp.py PARENT_LIB.so [NEW_LIB.so]          (NEW defaults to the tree's own library)
Each build runs in its own process (HDMOE_LIB_PATH) over every shape of tests/test_streaming_kernels.py and tests/test_conv7_addressing.py
with identical seeded operands:
  * y of hdmoe_conv_fwd, dx of the fused backward launch hdmoe_conv_bwd6, du and de of hdmoe_conv_bwd6_film: compared by SHA-256, must be equal;
  * the weight gradients of the fused backward launch (partial slabs, fp32 atomics in the flush where the path uses them): max |new - parent| must
    not exceed max |parent run 1 - parent run 2| of the same script.
Exit status 1 on any difference."""
import hashlib, importlib.util, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), ROOT]

FILM = [  # N, R, C, kernel sizes, segment ends (tests/test_film_dgrad_epilogue.py cases a - c, tests/test_conv7_addressing.py's FiLM case)
    (192, 32, 32, (3, 5, 3), (90, 90, 192)), (192, 32, 64, (3, 5, 3), (90, 90, 192)), (193, 16, 64, (3, 5, 3, 5), (51, 51, 100, 193)),
    (200, 32, 64, (3, 5), (97, 200)), (200, 16, 64, (3, 5), (97, 200)),
]


def shapes():
    out = {"fwd": [], "bwd": []}
    for f in ("test_streaming_kernels.py", "test_conv7_addressing.py"):
        spec = importlib.util.spec_from_file_location(f[:-3], os.path.join(ROOT, "tests", f))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        out["fwd"] += list(m.FWD); out["bwd"] += list(m.BWD)
    return out


def worker(outdir):
    import ctypes, torch
    from hdmoe_hip._lib import call, lib, _int_array
    from hdmoe_hip.bank import w6_record
    dev = "cuda"
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
    lines, grads = [], {}

    def weights(g, E, O, I, ks):
        ws = [(torch.randn(O, I, k, k, generator=g) / (I * k * k) ** 0.5).to(dev) for k in ks]
        taps, Opad = max(k * k for k in ks), (O + 15) // 16 * 16
        wstride, wdstride = taps * O * I, taps * I * Opad
        wf = torch.empty(E * wstride, dtype=torch.bfloat16, device=dev)
        wd = torch.empty(E * wdstride, dtype=torch.bfloat16, device=dev)
        call("hdmoe_wprep_fwd", ws, None, 1.0, list(ks), list(ks), E, O, I, I, Opad, wf, wstride, wd, wdstride, 0, 0, 1, 1)
        return wf, wstride, wd, wdstride

    def bwd(name, entry, x, dy, wd, wdstride, seg, N, R, I, O, ks, extra=()):
        """the fused backward launch twice -> (rc, dx, [Gs run 1, Gs run 2])"""
        E, pts = len(ks), [(k - 1) // 2 for k in ks]
        kib = lib().hdmoe_conv_wgrad6_ws_kib(E, N, R, R, I, O, ctypes.cast(_int_array(ks), ctypes.c_void_p), ctypes.cast(_int_array(ks), ctypes.c_void_p), 1)
        runs, dx, rc = [], None, 1
        for _ in range(2):
            if kib <= 0:
                break
            wsb = torch.zeros(2 * kib * 256, dtype=torch.float32, device=dev)
            Gs = [torch.zeros(k * k, O, I, device=dev) for k in ks]
            dx = torch.full_like(x, float("nan"))
            rc = call(entry, x, dy, wd, dx, Gs, seg, E, wdstride, N, R, R, I, O, list(ks), list(ks), pts, pts, 0.7, wsb, wsb.numel() * 4, *extra, 1)
            if rc != 0:
                break
            call("hdmoe_conv_wgrad6_reduce_batch", Gs + [None] * (8 - E), [seg], [wsb], w6_record(E, N, R, R, I, O, 1, ks), 1)
            torch.cuda.synchronize()
            runs.append(torch.cat([G.flatten() for G in Gs]).cpu())
        if runs:
            grads[name] = runs
        return rc, dx

    sh = shapes()
    for N, R, I, O, ks, split, res in sh["fwd"]:
        g = torch.Generator().manual_seed(N + R + I)
        E = len(ks)
        x = torch.randn(N, R, R, I, generator=g).bfloat16().to(dev)
        r = torch.randn(N, R, R, O, generator=g).bfloat16().to(dev) if res else None
        wf, wstride, _, _ = weights(g, E, O, I, ks)
        seg = torch.tensor([0] + list(split), dtype=torch.int32, device=dev)
        y = torch.full((N, R, R, O), float("nan"), dtype=torch.bfloat16, device=dev)
        pts = [(k - 1) // 2 for k in ks]
        rc = call("hdmoe_conv_fwd", x, wf, y, r, 0.7 if res else 1.0, 0.6 if res else 0.0, seg, E, wstride, N, R, R, R, R, I, I, I, O, O, 1, 0,
                  list(ks), list(ks), pts, pts, 1)
        lines.append(f"fwd N={N} R={R} {I}->{O} ks={ks} split={split} res={res}: rc {rc} y {sha(y)}")
    for N, R, I, O, ks, split in sh["bwd"] + [c[:6] for c in sh["fwd"]]:
        g = torch.Generator().manual_seed(N + R + O)
        x = torch.randn(N, R, R, I, generator=g).bfloat16().to(dev)
        dy = torch.randn(N, R, R, O, generator=g).bfloat16().to(dev)
        _, _, wd, wdstride = weights(g, len(ks), O, I, ks)
        seg = torch.tensor([0] + list(split), dtype=torch.int32, device=dev)
        name = f"bwd N={N} R={R} {I}->{O} ks={ks} split={split}"
        rc, dx = bwd(name, "hdmoe_conv_bwd6", x, dy, wd, wdstride, seg, N, R, I, O, ks)
        lines.append(f"{name}: rc {rc} dx {sha(dx) if rc == 0 else '-'}")
    for N, R, C, ks, split in FILM:
        g = torch.Generator().manual_seed(N + R + C)
        u = torch.randn(N, R, R, C, generator=g).bfloat16().to(dev)
        e = (1.0 + 0.3 * torch.randn(N, C, generator=g)).to(dev)
        dy = torch.randn(N, R, R, C, generator=g).bfloat16().to(dev)
        _, _, wd, wdstride = weights(g, len(ks), C, C, ks)
        seg = torch.tensor([0] + list(split), dtype=torch.int32, device=dev)
        h = torch.empty_like(u)
        mask = torch.zeros(u.numel() // 8, dtype=torch.uint8, device=dev)
        call("hdmoe_film_silu_drop_fwd_mask", h, mask, u, e, N, R * R, C, 0x1234567, None, 0.2, 1)
        de = torch.full_like(e, float("nan"))
        name = f"film N={N} R={R} C={C} ks={ks} split={split}"
        rc, du = bwd(name, "hdmoe_conv_bwd6_film", h, dy, wd, wdstride, seg, N, R, C, C, ks, extra=(u, e, mask, de, 0.2))
        lines.append(f"{name}: rc {rc} du {sha(du) if rc == 0 else '-'} de {sha(de) if rc == 0 else '-'}")
    open(os.path.join(outdir, "lines.txt"), "w").write("\n".join(lines) + "\n")
    torch.save(grads, os.path.join(outdir, "grads.pt"))


if __name__ == "__main__":
    if sys.argv[1] == "--worker":
        worker(sys.argv[2])
        sys.exit(0)
    import torch
    libs = [os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ""]
    res = []
    with tempfile.TemporaryDirectory() as d:
        for i, path in enumerate(libs):
            od = os.path.join(d, str(i)); os.mkdir(od)
            env = dict(os.environ)
            if path:
                env["HDMOE_LIB_PATH"] = path
            else:
                env.pop("HDMOE_LIB_PATH", None)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", od], env=env, check=True)
            res.append((open(os.path.join(od, "lines.txt")).read().splitlines(), torch.load(os.path.join(od, "grads.pt"))))
    (la, ga), (lb, gb) = res
    bad = 0
    print(f"== conv7_bitcmp: parent {os.path.relpath(libs[0], ROOT)}  against  {os.path.relpath(libs[1], ROOT) if libs[1] else 'the tree library'}")
    for a, b in zip(la, lb):
        same = a == b
        bad += not same
        print(("same " if same else "DIFF ") + a + ("" if same else "   |   new: " + b.split(": ", 1)[1]))
    for name in ga:
        own = float((ga[name][0] - ga[name][1]).abs().max())
        cross = float((gb[name][0] - ga[name][0]).abs().max()) if name in gb else float("inf")
        ok = cross <= own
        bad += not ok
        print(f"{'ok   ' if ok else 'DIFF '}wgrad {name}: max |new - parent| {cross:.3e}, parent run-to-run {own:.3e}")
    print("ALL IDENTICAL" if not bad and len(la) == len(lb) else f"{bad} DIFFERENCES")
    sys.exit(1 if bad or len(la) != len(lb) else 0)
