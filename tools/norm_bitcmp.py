"""Bit comparison of every entry point of csrc/norm.hip, and of hdmoe_gn_rag_fwd / _bwd of csrc/ragged.hip, between two builds of the library:
    python tools/norm_bitcmp.py PARENT_LIB.so [NEW_LIB.so]          (NEW defaults to the tree's own library)
Each build runs in its own process (HDMOE_LIB_PATH) with identical seeded operands and direct calls.  The shapes are the case tables of
tests/test_norm_kernels.py, the smallest that reach each dispatch path: ROW_CS at 1 and 70 rows and LONG_ROWS (the row kernels' grid caps),
GN_CASES, the row-range forms at the part counts ops.py picks and at parts = 64 over S = 130, the two bcast cases, FIN_CASES, GN1T_CASES, the
shapes of test_gn1t_act / test_gn1t_bwd; S = 1 rows for groupnorm_rows_bwd_kernel; one shape per GroupNorm arm just above its grid cap
(forward 16-byte arm 2048 workgroups, backward 16-byte arm 512, W = 1 arm 2048; gn1t_bwd 512, gn1t_act 1024); and per family one set of
operands that starts one element into its buffers (the row and GroupNorm entry points take their W = 1 arm, gn_rag has one arm, the
router-trunk entry points that check alignment must refuse: the refusal is the digest; hdmoe_gn1_*, which take aligned fp32 by contract
and do not check, get none).  fp32 and bf16 wherever the entry point takes a dtype.
Every output buffer starts as NaN (or the value the kernel adds to) with 8 guard elements on either side, and the whole buffer goes into
the SHA-256, so a write outside the output shows too.

Left out of the digests, because float atomics meet in them in an order the hardware picks (decided from the kernels' code; these outputs
stay under the fp64 bounds of tests/test_norm_kernels.py and tests/test_ragged_kernels.py):
  * hdmoe_layernorm_bwd dgamma / dbeta, both arms: atomicAdd into the workgroup's LDS partials sm[2 C], then one global atomic per workgroup;
  * hdmoe_groupnorm_bwd* on the W = 1 arm (groupnorm_bwd_stats_kernel) dgamma / dbeta: atomicAdd into LDS sm[2 C];
  * hdmoe_gn_rag_bwd dgamma / dbeta: atomicAdd into LDS sm[2 C], then global atomics from every row's workgroup;
  * hdmoe_groupnorm_bwd* on the 16-byte arm and hdmoe_gn1t_bwd (groupnorm_bwd_stats_vec_kernel) dgamma / dbeta: one global atomicAdd per
    channel and workgroup -- taken where N * parts == 1, left out otherwise;
  * hdmoe_groupnorm_bwd on S = 1 rows (groupnorm_rows_bwd_kernel) dgamma / dbeta: one global atomicAdd per channel and workgroup of 8 rows
    -- taken where N <= 8;
  * hdmoe_groupnorm_bwd_split s1 / s2 (atomicAdd of every row range's sum into the zeroed ws) with more than two non-empty row ranges,
    and the dx computed from them: two addends commute, three do not associate.  (Nothing of that call is left then: it is not made.)
Prints both digest lists and the verdict; exit status 1 on any difference, 2 when a run did not finish."""
import hashlib, math, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), ROOT]

ROW_CS = [1, 3, 4, 8, 12, 16, 24, 30, 36, 40, 72, 132, 256, 260, 264, 512, 520]
LONG_ROWS = [(16400, 256), (2100, 256), (524300, 3)]
GN_CASES = [(2, 5, 8, 1, 1), (2, 7, 24, 8, 0), (3, 33, 32, 8, 2), (1, 9, 256, 64, 0), (1, 9, 512, 64, 2), (1, 3, 2048, 1, 1), (2, 2, 4096, 32, 2),
            (4, 1, 8, 8, 0), (2, 513, 16, 2, 2), (3, 1023, 32, 4, 0), (1, 1025, 8, 1, 1), (130, 256, 8, 1, 2)]
GN_ROWS = [(5, 1, 512, 1, 1), (9, 1, 1000, 1, 2)]                                   # S = 1, G = 1: groupnorm_rows_bwd_kernel<2>, <4> in fp32
GN_CAPS = [(1, 65540, 32, 4, 2), (1, 65540, 64, 4, 2), (1, 16400, 32, 4, 2), (1, 16400, 64, 4, 2), (1, 21850, 24, 8, 2)]
GN_SPLIT = [(2, 513, 16, 2, 2, 2, 4), (2, 513, 16, 2, 2, 2, 2), (3, 1023, 32, 4, 0, 3, 7), (1, 1025, 8, 1, 1, 4, 8), (2, 130, 16, 2, 2, 64, 64)]
FIN_CASES = [(3, 1, 1, 4), (2, 65, 700, 4), (2, 64, 170, 4), (2, 64, 3, 24), (2, 65, 170, 24), (2, 130, 700, 24), (2, 1, 170, 128),
             (2, 130, 1, 128), (1, 130, 3, 1024), (1, 64, 37, 1024)]
GN1T_CASES = [(1, 1, 8, 8), (3, 15, 24, 40), (2, 127, 16, 8), (2, 128, 16, 8), (2, 129, 16, 8), (1, 2049, 8, 16), (65, 17, 24, 24), (1, 2, 2048, 8),
              (2, 300, 16, 8)]
GN1T_BWD = [(3, 50, 4), (2, 37, 64), (1, 5, 2048), (1, 16400, 32)]                   # the last: 513 workgroups wanted, 512 launched
GN1T_ACT = [(2, 19, 8), (2, 19, 24), (1, 16400, 128)]                                # the last: 1025 wanted, 1024 launched
RAG_CASES = [([5, 3], [0, 2, 3], 4, 32, 4), ([5, 3], [0, 2, 3], 4, 24, 8), ([40, 17], [0, 1, 3], 3, 32, 4), ([7, 7, 2], [0, 1, 2, 4], 4, 8, 1)]
EPS = 1e-5


def worker(path):
    import torch
    from hdmoe_hip._lib import call
    F32, BF16, dev, GD = torch.float32, torch.bfloat16, "cuda", 8
    lines = []
    gen = torch.Generator().manual_seed(20240917)

    def rnd(shape, dtype=F32, off=0, mean=0.3, std=1.3):      # seeded values, `off` elements into their buffer
        n = math.prod(shape)
        return (torch.randn(n + off, generator=gen) * std + mean).to(dtype).to(dev)[off:].view(shape)

    def out(shape, dtype=F32, off=0, fill=float("nan")):      # (whole buffer with guards, the view the kernel writes)
        n = math.prod(shape)
        b = torch.full((n + 2 * GD + off,), fill, dtype=dtype, device=dev)
        return b, b[GD + off:GD + off + n].view(shape)

    def emit(name, *bufs):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for b in bufs:
            h.update(b.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        lines.append(f"{name}: {h.hexdigest()[:16]}")

    def refused(name, fn):
        try:
            fn()
            torch.cuda.synchronize()
            lines.append(f"{name}: taken")
        except RuntimeError as e:
            lines.append(f"{name}: refused ({str(e).split(': ')[-1]})")

    def affine(C):
        return rnd((C,), mean=1.0, std=0.3), rnd((C,), mean=0.0, std=0.2)

    for dtype, dt, W, tag in ((F32, 0, 4, "fp32"), (BF16, 1, 8, "bf16")):
        # ---- 1. row kernels
        for rows, C, off in [(r, C, 0) for r in (1, 70) for C in ROW_CS] + [(r, C, 0) for r, C in LONG_ROWS] + [(70, 32, 1)]:
            sfx = f"rows={rows} C={C} off={off} [{tag}]"
            x, dxn, dh, (gm, bt) = rnd((rows, C), dtype, off), rnd((rows, C), dtype, off), rnd((rows, C), dtype, off), affine(C)
            xb, xn = out((rows, C), dtype, off); hb, h = out((rows, C), dtype, off)
            call("hdmoe_pixelnorm_fwd", xn, h, x, rows, C, dt); emit(f"pixelnorm_fwd {sfx}", xb, hb)
            xb, xn = out((rows, C), dtype, off)
            call("hdmoe_pixelnorm_fwd", xn, None, x, rows, C, dt); emit(f"pixelnorm_fwd h=NULL {sfx}", xb)
            for a, b, what in ((dxn, dh, ""), (None, dh, " dxn=NULL"), (dxn, None, " dh=NULL")):
                db_, dx = out((rows, C), dtype, off)
                call("hdmoe_pixelnorm_bwd", dx, a, b, x, rows, C, 0.3, dt); emit(f"pixelnorm_bwd{what} {sfx}", db_)
            yb, y = out((rows, C), dtype, off); mb, mean = out((rows,)); rb, rstd = out((rows,))
            call("hdmoe_layernorm_fwd", y, mean, rstd, x, gm, bt, rows, C, EPS, dt); emit(f"layernorm_fwd {sfx}", yb, mb, rb)
            db_, dx = out((rows, C), dtype, off); dg, dbt = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            call("hdmoe_layernorm_bwd", dx, dg, dbt, dxn, x, gm, mean, rstd, rows, C, dt); emit(f"layernorm_bwd dx {sfx}", db_)

        # ---- 2. GroupNorm
        def gn_arm(N, S, C, G, off):
            if dtype == F32 and S == 1 and G == 1 and C % 4 == 0 and C <= 1024 and off == 0:
                return "rows"
            cv = C // W
            return "vec" if C % W == 0 and (C // G) % W == 0 and cv <= 512 and 512 % cv == 0 and off == 0 else "w1"

        for (N, S, C, G, act), off in [(c, 0) for c in GN_CASES + GN_ROWS + GN_CAPS] + [((2, 33, 32, 4, 2), 1)]:
            sfx = f"{(N, S, C, G, act)} off={off} [{tag}]"
            x, dy, (gm, bt) = rnd((N, S, C), dtype, off), rnd((N, S, C), dtype, off, 0.25, 1.0), affine(C)
            yb, y = out((N, S, C), dtype, off); mb, mean = out((N * G,)); rb, rstd = out((N * G,))
            call("hdmoe_groupnorm_fwd", y, mean, rstd, x, gm, bt, N, S, C, G, act, EPS, dt); emit(f"groupnorm_fwd {sfx}", yb, mb, rb)
            db_, dx = out((N, S, C), dtype, off); wb, ws = out((2 * N * G,)); gb, dg = out((C,), fill=0.25); bb, dbt = out((C,), fill=-0.5)
            call("hdmoe_groupnorm_bwd", dx, dg, dbt, ws, dy, x, gm, bt, mean, rstd, N, S, C, G, act, dt)
            arm = gn_arm(N, S, C, G, off)
            par = (arm == "vec" and N == 1) or (arm == "rows" and N <= 8)
            emit(f"groupnorm_bwd {arm}{' +dgamma/dbeta' if par else ''} {sfx}", db_, *([] if arm == "rows" else [wb]), *([gb, bb] if par else []))
        for N, S, C, G, act, fparts, bparts in GN_SPLIT:
            sfx = f"{(N, S, C, G, act)} [{tag}]"
            assert gn_arm(N, S, C, G, 0) == "vec"
            x, dy, (gm, bt) = rnd((N, S, C), dtype), rnd((N, S, C), dtype, 0, 0.25, 1.0), affine(C)
            yb, y = out((N, S, C), dtype); mb, mean = out((N * G,)); rb, rstd = out((N * G,)); wb, ws = out((2 * N * fparts * G,))
            call("hdmoe_groupnorm_fwd_split", y, mean, rstd, ws, fparts, x, gm, bt, N, S, C, G, act, EPS, dt)
            emit(f"groupnorm_fwd_split parts={fparts} {sfx}", yb, mb, rb, wb)
            rpp = (S + bparts - 1) // bparts
            if sum(1 for p in range(bparts) if min(p * rpp, S) < min(p * rpp + rpp, S)) > 2:
                continue
            db_, dx = out((N, S, C), dtype); wb, ws = out((2 * N * G,), fill=0.0); dg, dbt = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            call("hdmoe_groupnorm_bwd_split", dx, dg, dbt, ws, bparts, dy, x, gm, bt, mean, rstd, N, S, C, G, act, dt)
            emit(f"groupnorm_bwd_split parts={bparts} {sfx}", db_, wb)
        for N, S, C in ((3, 40, 16), (65, 17, 32)):
            sfx = f"{(N, S, C)} [{tag}]"
            x, g, (gm, bt) = rnd((N, S, C), dtype), rnd((N, C), F32, 0, 0.25, 1.0), affine(C)
            yb, y = out((N, S, C), dtype); mb, mean = out((N,)); rb, rstd = out((N,))
            call("hdmoe_groupnorm_fwd", y, mean, rstd, x, gm, bt, N, S, C, 1, 1, EPS, dt)
            db_, dx = out((N, S, C), dtype); wb, ws = out((2 * N,)); dg, dbt = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            call("hdmoe_groupnorm_bwd_bcast", dx, dg, dbt, ws, g, 1.0 / S, x, gm, bt, mean, rstd, N, S, C, 1, 1, dt)
            emit(f"groupnorm_bwd_bcast {sfx}", yb, mb, rb, db_, wb)
        x1 = rnd((2, 40, 30), dtype)                           # C % W != 0: the broadcast form has no W = 1 arm
        refused(f"groupnorm_bwd_bcast C=30 [{tag}]", lambda: call("hdmoe_groupnorm_bwd_bcast", out((2, 40, 30), dtype)[1], torch.zeros(30, device=dev),
                torch.zeros(30, device=dev), out((4,))[1], rnd((2, 30)), 0.025, x1, *affine(30), rnd((2,)), rnd((2,)), 2, 40, 30, 1, 1, dt))

        # ---- 3. ragged GroupNorm (ragged.hip)
        for (lens, seg, R, C, G), off in [(c, 0) for c in RAG_CASES] + [(RAG_CASES[0], 1)]:
            Sp, ng = max(lens), len(lens)
            segd = torch.tensor(seg, dtype=torch.int32, device=dev)
            for act in (0, 1, 2):
                sfx = f"lens={lens} seg={seg} R={R} C={C} G={G} act={act} off={off} [{tag}]"
                x, dy = rnd((R, Sp, C), dtype, off), rnd((R, Sp, C), dtype, off, 0.25, 1.0)
                gms, bts = [affine(C)[0] for _ in range(ng)], [affine(C)[1] for _ in range(ng)]
                yb, y = out((R, Sp, C), dtype, off); mb, mean = out((R * G,)); rb, rstd = out((R * G,))
                call("hdmoe_gn_rag_fwd", y, mean, rstd, x, gms, bts, segd, lens, ng, R, Sp, C, G, act, EPS, dt); emit(f"gn_rag_fwd {sfx}", yb, mb, rb)
                db_, dx = out((R, Sp, C), dtype, off)
                dgs, dbs = [torch.zeros(C, device=dev) for _ in range(ng)], [torch.zeros(C, device=dev) for _ in range(ng)]
                call("hdmoe_gn_rag_bwd", dx, dgs, dbs, dy, x, gms, bts, mean, rstd, segd, lens, ng, R, Sp, C, G, act, dt); emit(f"gn_rag_bwd dx {sfx}", db_)

    # ---- 4. router-trunk family (fp32 activations, bf16 gradients)
    def stats_of(y):
        yd = y.cpu().double().reshape(y.shape[0], -1)            # (on the CPU: operands must not depend on a device reduction's order)
        return yd.mean(1).float().to(dev), (yd.var(1, unbiased=False) + EPS).rsqrt().float().to(dev)

    for N, slots, S, C in FIN_CASES:
        sfx = f"{(N, slots, S, C)}"
        y, (gm, bt) = rnd((N, S, C), F32, 0, 0.4, 1.7), affine(C)
        ch = torch.tensor_split(y.cpu().double().reshape(N, -1), slots, dim=1)
        ws = torch.stack([torch.stack([c.sum(1), c.square().sum(1)], -1) for c in ch], 1).float().contiguous().to(dev)
        sb, sc = out((N, C)); hb, sh = out((N, C)); mb, mean = out((N,)); rb, rstd = out((N,))
        call("hdmoe_gn1_finalize", sc, sh, mean, rstd, ws, gm, bt, N, slots, C, S * C, EPS); emit(f"gn1_finalize {sfx}", sb, hb, mb, rb)
        ob, o = out((N, C))
        call("hdmoe_gn1_relu_mean", o, y, sc.contiguous(), sh.contiguous(), N, S, C); emit(f"gn1_relu_mean {sfx}", ob)
        ob, o = out((N, C)); sb, sc = out((N, C)); hb, sh = out((N, C)); mb, mean = out((N,)); rb, rstd = out((N,))
        call("hdmoe_gn1_finalize_relu_mean", o, sc, sh, mean, rstd, y, ws, gm, bt, N, slots, S, C, EPS); emit(f"gn1_finalize_relu_mean {sfx}", ob, sb, hb, mb, rb)
        ob, o = out((N, C)); sb, sc = out((N, C)); hb, sh = out((N, C)); mb, mean = out((N,)); rb, rstd = out((N,)); pb, P = out((N, C)); qb, Q = out((N, C))
        call("hdmoe_gn1_finalize_relu_mean_pq", o, sc, sh, mean, rstd, P, Q, y, ws, gm, bt, N, slots, S, C, EPS)
        emit(f"gn1_finalize_relu_mean_pq {sfx}", ob, sb, hb, mb, rb, pb, qb)
    for N, S, C in GN1T_ACT:
        y, sc, sh = rnd((N, S, C), F32, 0, -0.1, 1.3), rnd((N, C), F32, 0, 1.0, 0.2), rnd((N, C), F32, 0, 0.0, 0.3)
        ob, o = out((N, S, C), BF16); call("hdmoe_gn1t_act", o, y, sc, sh, N, S, C); emit(f"gn1t_act {(N, S, C)}", ob)
        ob, o = out((N, S, C), BF16); call("hdmoe_gn1t_act", o, y, None, None, N, S, C); emit(f"gn1t_act scale=NULL {(N, S, C)}", ob)
    for N, S, C in GN1T_BWD:
        y, dz, g, (gm, bt) = rnd((N, S, C), F32, 0, 0.4, 1.7), rnd((N, S, C), BF16, 0, 0.25, 1.0), rnd((N, C), F32, 0, 0.25, 1.0), affine(C)
        mean, rstd = stats_of(y)
        for form, a, b, gs in (("dz", dz, None, 1.0), ("g", None, g, 1.0 / S)):
            db_, dx = out((N, S, C), BF16); wb, ws = out((2 * N,)); gb, dg = out((C,), fill=0.25); bb, dbt = out((C,), fill=-0.5)
            call("hdmoe_gn1t_bwd", dx, dg, dbt, ws, a, b, gs, y, gm, bt, mean, rstd, N, S, C)
            emit(f"gn1t_bwd {form}{' +dgamma/dbeta' if N == 1 else ''} {(N, S, C)}", db_, wb, *([gb, bb] if N == 1 else []))
    for N, S, C, CI in GN1T_CASES:
        y, dz, g, (gm, bt) = rnd((N, S, C), F32, 0, 0.4, 1.7), rnd((N, S, C), BF16, 0, 0.25, 1.0), rnd((N, C), F32, 0, 0.25, 1.0), affine(C)
        xin, isc, ish = rnd((N, S, CI), F32, 0, -0.1, 1.3), rnd((N, CI), F32, 0, 1.0, 0.2), rnd((N, CI), F32, 0, 0.0, 0.3)
        mean, rstd = stats_of(y)
        xh = (y.cpu() - mean.cpu().view(N, 1, 1)) * rstd.cpu().view(N, 1, 1)
        opn = (xh * gm.cpu() + bt.cpu()) > 0
        pcnt, qsum = opn.float().sum(1).to(dev), (xh * opn).sum(1).to(dev)
        parts = max(1, min(16, S // 128))
        wb, ws = out((2 * N * parts * (1 + C),))
        call("hdmoe_gn1t_stats", ws, dz, y, gm, bt, mean, rstd, N, S, C); emit(f"gn1t_stats {(N, S, C)}", wb)
        for form in ("dz", "pooled"):
            for sc_, sh_, what in ((isc, ish, ""), (None, None, " scale=NULL")):
                db_, dx = out((N, S, C), BF16); ab, a = out((N, S, CI), BF16); gb, dg = out((C,), fill=0.25); bb, dbt = out((C,), fill=-0.5)
                if form == "dz":
                    call("hdmoe_gn1t_apply", dx, a, dg, dbt, ws, dz, None, 1.0, None, None, y, gm, bt, mean, rstd, xin, sc_, sh_, N, S, C, CI)
                else:
                    call("hdmoe_gn1t_apply", dx, a, dg, dbt, None, None, g, 1.0 / S, pcnt, qsum, y, gm, bt, mean, rstd, xin, sc_, sh_, N, S, C, CI)
                emit(f"gn1t_apply {form}{what} {(N, S, C, CI)}", db_, ab, gb, bb)
    N, S, C = 2, 19, 8                                         # operands one element into their buffers: every checking entry point refuses
    y1, dz1, (gm, bt), m1, r1 = rnd((N, S, C), F32, 1), rnd((N, S, C), BF16, 1), affine(C), rnd((N,)), rnd((N,))
    o1, w1, z = out((N, S, C), BF16)[1], out((2 * N * (1 + C),))[1], torch.zeros(C, device=dev)
    refused("gn1t_act off=1", lambda: call("hdmoe_gn1t_act", o1, y1, None, None, N, S, C))
    refused("gn1t_bwd off=1", lambda: call("hdmoe_gn1t_bwd", o1, z, z.clone(), w1, dz1, None, 1.0, y1, gm, bt, m1, r1, N, S, C))
    refused("gn1t_stats off=1", lambda: call("hdmoe_gn1t_stats", w1, dz1, y1, gm, bt, m1, r1, N, S, C))
    refused("gn1t_apply off=1", lambda: call("hdmoe_gn1t_apply", o1, out((N, S, C), BF16)[1], z, z.clone(), w1, dz1, None, 1.0, None, None, y1, gm, bt, m1, r1,
                                              y1, None, None, N, S, C, C))
    open(path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "--worker":
        worker(sys.argv[2])
        sys.exit(0)
    libs = [os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ""]
    res = []
    with tempfile.TemporaryDirectory() as d:
        for i, path in enumerate(libs):
            env = dict(os.environ)
            if path:
                env["HDMOE_LIB_PATH"] = path
            else:
                env.pop("HDMOE_LIB_PATH", None)
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", os.path.join(d, str(i))], env=env).returncode
            if rc:
                print(f"the run of {path or 'the tree library'} ended with status {rc}: nothing compared")
                sys.exit(2)
            res.append(open(os.path.join(d, str(i))).read().splitlines())
    la, lb = res
    print(f"== norm_bitcmp: parent {os.path.relpath(libs[0], ROOT)}  against  {os.path.relpath(libs[1], ROOT) if libs[1] else 'the tree library'}")
    print(f"-- parent digests ({len(la)})"); print("\n".join(la))
    print(f"-- new digests ({len(lb)})"); print("\n".join(lb))
    diff = [(a, b) for a, b in zip(la, lb) if a != b]
    for a, b in diff:
        print(f"DIFF {a}   |   new: {b.rsplit(': ', 1)[1]}")
    ok = not diff and len(la) == len(lb)
    print(f"ALL {len(la)} IDENTICAL" if ok else f"{len(diff)} DIFFERENCES")
    sys.exit(0 if ok else 1)
