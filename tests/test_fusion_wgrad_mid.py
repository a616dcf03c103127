"""Weight gradients inside the fused backward kernels of the fusion stage (csrc/fusion.hip: hdmoe_fusion_in_bwd_wg,
hdmoe_fusion_out_bwd_wg), the forward that no longer writes cat / s, the chain between the two attention cores (hdmoe_fusion_mid_fwd /
_bwd) and the text attention's k / v projections in one launch per direction (csrc/kgemm.hip hdmoe_kgemm2_fwd, csrc/lwgrad.hip
hdmoe_lwgrad2) -- GPU.

What is compared with what.
  bf16 outputs (dfu, dfv; do2, da, dU; mixed, a2, g1 of the forward called with cat = s = NULL): bit-equal to the entry points without
  `_wg`, called directly on the same buffers.  The arithmetic is one templated body, so any difference is a bug.
  fp32 reductions that both forms make with atomics (dsw, dalpha): both are fp32 sums of the SAME terms (the terms are formed by the same
  code from bit-equal operands) in another order, each within the reduction bound of tests/test_elementwise_kernels.py,
  8 u (|r| + sum |terms|), u = 2^-24, of the float64 sum r -- so they may differ by twice that.
  weight-gradient slabs: G += dy^T x against the float64 contraction of the same bf16 operands (dy = dq / dk / dv as passed in, or dat /
  dg1 / dl as hdmoe_fusion_out_bwd stores them; x = query / ctx of hdmoe_fusion_in_fwd, or o2 / cat / s of hdmoe_fusion_out_fwd).  The
  bound is measured, not chosen: the existing weight-only launch (hdmoe_conv_wgrad, what ops.py called for these layers before) runs on
  the same operands into a slab with the same non-zero prefill, and the new kernel's worst error may be at most twice that launch's own
  worst error (both sum in fp32 in a free order; two is the spread between two such orders -- the rule of tests/test_pointwise_bwd.py).
  Where that launch meets float64 exactly, one fp32 ulp of the slab's largest element is allowed.  The prefill (multiples of 1/4) shows
  that the kernels add to the slab; both errors of every case are printed and written to profiles/fusion_wg_errors.json.

Shapes.  What can go wrong is the tile tail and the grid-stride loop, so the workgroup cap argument is 2 (8 waves) and rows are 1 (no
full tile), 31, 32 (one tile, exact), 33 (a tile and a tail), 255, 256 (one tile per wave), 257, and 8 * 32 * 2 + 17 = 529 (waves with
two tiles, then a partial tile).  A row past the end is a copy of the last row in the kernel's registers: it must add exactly nothing,
which the float64 comparison at rows = 1 would show 31-fold.  The in chain runs once more as 3 samples of 100 rows, so that sw / dsw
change inside a tile, and once without sw (query, ctx = fu, fv).  Every output and slab sits between guard elements, compared bit for
bit; inputs must be unchanged.  A misaligned base, fp32 tensors or 64 channels are refused (return 1) with nothing written.

Mid chain.  hdmoe_fusion_mid_fwd / _bwd against the launches they replace, called directly: hdmoe_conv_fwd with the residual epilogue and
hdmoe_conv_fwd (a, q2); hdmoe_pw_bwd on q_proj, torch's bf16 `+` (the add autograd makes for a's two gradients), hdmoe_pw_bwd on
out_proj and hdmoe_axpby (do1, dres): all four bf16 outputs bit-equal, at the rows above with the cap of 2, with and without slabs; the
two slabs under the slab rule with dy = dq2 / the unfused chain's da_t and x = its a / o1.

Paired k / v projections.  hdmoe_kgemm2_fwd against two hdmoe_conv_fwd calls (the long-contraction kernel) on the same x and images: k and
v bit-equal.  A workgroup owns 32 rows and its eight waves split K in 64-element chunks, two buffers deep: rows 1, 31, 32, 33, 257 and
K = 512 (one chunk per wave), 768 (the text width: waves with two chunks and with one), 1088 (17 chunks: a third trip).  hdmoe_lwgrad2
against float64 and two hdmoe_conv_wgrad launches under the slab rule above; a wave takes 64-row slices: rows 1, 63, 64, 65, 257, 1000.

Model level: _fusion_tail forward + backward at B = 2 (2048 rows) on the wide_config1 fixture's weights with ops.FUSION_FUSED on and off.
The fused kernels round to bf16 wherever the unfused ops store a tensor, so out, gate, d out_u and d out_v are asserted bit-equal; every
dy and x of the ten layers is then the same bf16 data on both paths and what is left differs by fp32 summation order alone.  At this size
the slab errors of BOTH paths are one to three fp32 ulps of the slab's largest element and move with the order of the atomics from run
to run, and several tensors of the unfused path come out the same in every run, so neither "twice the other launch's worst error" nor
"twice the distance between two unfused runs" is a stable measure here (measured: either fails on one tensor in ten, another one each
run).  The bounds are therefore the a-priori one this suite uses for fp32 reductions (tests/test_elementwise_kernels.py,
tests/test_fusion_stage_kernels.py): an fp32 sum r of terms t_i, in any order, within 8 u (|r| + sum |t_i|), u = 2^-24, with the terms
taken from the UNFUSED run's launch arguments (reference data, never the fused path's results):
  slabs: the step's C-ABI calls are intercepted; after each weight-gradient launch the bank's real slab is copied (the bank zeroes the slabs
    at the start of a step and each layer adds once), and the unfused launches (hdmoe_pw_bwd, hdmoe_conv_wgrad) also give the layer's x and
    dy.  Every element of both paths' slab, matched to its layer by parameter identity through the bank's entries, must lie within
    8 u (|r| + (|dy|^T |x|)) of r = (dy^T x) in float64.  A dropped or doubled 32-row tile is ~5 sigma of a term against ~1e-3 sigma of
    bound, a slab of another layer or a misplaced element likewise.
  parameter gradients of the ten layers: the bank's finish launch, the same deterministic launch on both paths, applied to those slabs;
    |fused - unfused| <= 2 * 8 u (1 + kappa) max|unfused|, kappa = max(|dy|^T |x|) / max|r| of the layer's slab (the slab's bound relative to
    its largest element, once per path).
  alpha_txt.grad = dalpha: |fused - unfused| <= 2 * 8 u (|r| + sum |t|), t = da2 (at - a) from hdmoe_lerp_param_bwd's arguments.
  d s_vit, d s_unet: elementwise linear in dsw[n] (sigmoid backward, two axpby: 4 u for their roundings), so per sample
    |fused - unfused| <= |unfused| (2 * 8 u (|r_n| + sum |t_n|) / |r_n| + 4 u), t = dd t from hdmoe_scale_rows_bwd's arguments.
All of these are four to five orders of magnitude below the 6e-2 end-to-end tolerance of tests/test_fusion_stage_kernels.py.
The call log of the fused step has one hdmoe_fusion_in_bwd_wg and one hdmoe_fusion_out_bwd_wg, one hdmoe_fusion_mid_fwd / _bwd (the
selection counters fusion_mid, fusion_mid_bwd advance), one hdmoe_kgemm2_fwd and one hdmoe_lwgrad2, no hdmoe_pw_bwd, and no weight-only
launch for their ten layers: hdmoe_conv_wgrad is called for output_proj only.
"""
import json
import os

import pytest
import torch

import test_fusion_stage_kernels as K
from test_fusion_stage_kernels import BF16, DEV, F32, FILL, Guarded, U as ULP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [1, 31, 32, 33, 255, 256, 257, 8 * 32 * 2 + 17]
CAP = 2                                                      # workgroups: 8 waves, so 529 rows = 17 tiles take the grid-stride loop
GUARD_F = 16                                                 # guard floats on either side of a slab
ERRORS = {}


@pytest.fixture(scope="module")
def call():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    yield call
    if ERRORS:
        try:                                                     # (a read-only checkout keeps the committed figures)
            with open(os.path.join(ROOT, "profiles", "fusion_wg_errors.json"), "w") as f:
                json.dump(ERRORS, f, indent=1, sort_keys=True)
        except OSError:
            pass


class Slab:
    """An fp32 [O][I] slab with a non-zero prefill between GUARD_F guard floats."""

    def __init__(self, O, I):
        self.buf = torch.full((O * I + 2 * GUARD_F,), FILL, dtype=F32, device=DEV)
        self.t = self.buf[GUARD_F:GUARD_F + O * I]
        self.fill = (0.25 * ((torch.arange(O * I, device=DEV) % 7) - 3)).to(F32)
        self.t.copy_(self.fill)
        self.O, self.I = O, I

    def guards_intact(self):
        return bool((self.buf[:GUARD_F] == FILL).all() and (self.buf[-GUARD_F:] == FILL).all())


def _wgrad_old(call, x, dy, rows, I, O):
    """The weight-only launch ops.py made for the layer, into a slab with the same prefill."""
    s = Slab(O, I)
    call("hdmoe_conv_wgrad", x, dy, [s.t], None, 1, 1, 1, rows, 1, rows, I, I, O, 1, 0, [1], [1], [0], [0], 1)
    return s


def _check_slab(tag, new, old, x, dy):
    """new / old: Slabs after the fused kernel / after hdmoe_conv_wgrad; x (rows, I), dy (rows, O) the bf16 operands."""
    assert new.guards_intact() and old.guards_intact(), f"{tag}: guard floats of a slab overwritten"
    ref = new.fill.double() + (dy.double().t() @ x.double()).reshape(-1)
    en = float((new.t.double() - ref).abs().max())
    eo = float((old.t.double() - ref).abs().max())
    mx = float(ref.abs().max())
    ulp = 2.0 ** (torch.tensor(mx).log2().floor().item() - 23)
    bound = 2.0 * eo if eo > 0.0 else ulp
    print(f"{tag}: max|ref| {mx:.3e}  hdmoe_conv_wgrad err {eo:.3e}  in-kernel err {en:.3e}  bound {bound:.3e}")
    ERRORS[tag] = dict(max_ref=mx, conv_wgrad_err=eo, in_kernel_err=en, bound=bound)
    assert torch.isfinite(new.t).all() and en <= bound, (tag, en, eo, bound)


def _bits(t):
    return t.contiguous().view(torch.int16)


IN_CASES = [(1, r, True) for r in ROWS] + [(3, 100, True), (1, 257, False)]


@pytest.mark.parametrize("B,S,use_sw", IN_CASES, ids=[f"B{B}-S{S}-{'sw' if w else 'nosw'}" for B, S, w in IN_CASES])
def test_in_backward_with_weight_gradients(call, B, S, use_sw):
    d, T, W, sw, rows = K._setup(B, S, 4000 * B + S)
    sw = sw if use_sw else None
    plain = K._fused(call, T, W, sw, rows, S, True)               # hdmoe_fusion_in_fwd + hdmoe_fusion_in_bwd, guards checked
    query, ctx = (plain["query"], plain["ctx"]) if use_sw else (T["fu"].t, T["fv"].t)
    o = {n: Guarded(rows) for n in ("dfu", "dfv")}
    G = [Slab(32, 32) for _ in range(3)]
    dsw = torch.zeros(B + 2, dtype=F32, device=DEV) if use_sw else None
    rc = call("hdmoe_fusion_in_bwd_wg", T["dq"].t, T["dk"].t, T["dv"].t, T["gquery"].t, T["gctx"].t, T["fu"].t, T["fv"].t, sw, W["wdq"], W["wdk"],
              W["wdv"], o["dfu"].t, o["dfv"].t, dsw[1:-1] if use_sw else None, G[0].t, G[1].t, G[2].t, CAP, rows, S, 32, 1.0, 1.0, 1.0, 1)
    assert rc == 0, "hdmoe_fusion_in_bwd_wg declined a shape of its domain"
    torch.cuda.synchronize()
    for n, gt in T.items():
        assert gt.unchanged(), f"input {n} or its guard rows changed"
    for n, gt in o.items():
        assert gt.guards_intact(), f"guard rows of {n} overwritten"
        assert torch.equal(_bits(gt.t), _bits(plain[n])), f"{n}: differs from hdmoe_fusion_in_bwd's"
    tag = f"in B={B} S={S} sw={use_sw}"
    if use_sw:
        assert float(dsw[0]) == 0.0 and float(dsw[-1]) == 0.0, "dsw written out of range"
        ref = K._reference(d, B, S, True, True)
        diff = (dsw[1:-1].cpu().double() - plain["dsw"].cpu().double()).abs()
        bound = 2 * 8 * ULP * (ref["dsw"].abs() + ref["dsw_scale"]) + 2.0 ** -126
        print(f"{tag} dsw: worst |wg - plain| / bound {float((diff / bound).max()):.3f}")
        assert bool((diff <= bound).all()), (diff, bound)
    for g, name, x, dy in zip(G, ("q_proj", "k_proj", "v_proj"), (query, ctx, ctx), (T["dq"].t, T["dk"].t, T["dv"].t)):
        _check_slab(f"{tag} {name}", g, _wgrad_old(call, x.contiguous(), dy, rows, 32, 32), x, dy)


def _out_wg(call, T, W, dgate, alpha, rows, saved):
    o = {n: Guarded(rows) for n in ("do2", "da", "dU")}
    G = [Slab(32, 32), Slab(32, 64), Slab(2, 32)]
    dal = torch.zeros(3, dtype=F32, device=DEV)
    rc = call("hdmoe_fusion_out_bwd_wg", T["dmixed"].t, dgate, saved["gate"], T["U"].t, saved["a2"], saved["g1"], T["o2"].t, T["a"].t, alpha,
              W["wo"], W["wdo"], W["wd1"], W["wd2"], o["do2"].t, o["da"].t, o["dU"].t, dal[1:2], G[0].t, G[1].t, G[2].t, CAP, rows, 32,
              K.AO, K.BO, K.WA, K.WB, 1.0, 1.0, 1)
    assert rc == 0, "hdmoe_fusion_out_bwd_wg declined a shape of its domain"
    torch.cuda.synchronize()
    assert float(dal[0]) == 0.0 and float(dal[2]) == 0.0, "dalpha written out of range"
    return o, G, dal[1:2].clone()


OUT_CASES = [(r, True) for r in ROWS] + [(257, False)]


@pytest.mark.parametrize("rows,use_dgate", OUT_CASES, ids=[f"rows{r}-{'dgate' if g else 'nodgate'}" for r, g in OUT_CASES])
def test_out_backward_with_weight_gradients(call, rows, use_dgate):
    d, T, W, dgate, alpha = K._out_setup(rows, 17 * rows + 3)
    dg = dgate if use_dgate else None
    plain = K._out_fused(call, T, W, dg, alpha, rows)             # hdmoe_fusion_out_fwd (all four saved tensors) + hdmoe_fusion_out_bwd
    # the forward with cat = s = NULL writes the same mixed, gate, a2, g1 (and has nowhere to write the other two)
    f = {n: Guarded(rows) for n in ("mixed", "a2", "g1")}
    gate = torch.full((rows + 2, 2), FILL, dtype=F32, device=DEV)
    k = (32, K.AO, K.BO, K.WA, K.WB, 1.0, 1.0, 1)
    assert call("hdmoe_fusion_out_fwd", T["o2"].t, T["a"].t, T["U"].t, alpha, W["wo"], W["w1"], W["w2"], f["mixed"].t, gate[1:-1], f["a2"].t,
                f["g1"].t, None, None, rows, *k) == 0, "hdmoe_fusion_out_fwd declined a2, g1 without cat, s"
    torch.cuda.synchronize()
    for n, gt in f.items():
        assert gt.guards_intact() and torch.equal(_bits(gt.t), _bits(plain[n])), f"forward without cat / s: {n} differs"
    assert bool((gate[0] == FILL).all() and (gate[-1] == FILL).all()) and torch.equal(gate[1:-1], plain["gate"])
    o, G, dal = _out_wg(call, T, W, dg, alpha, rows, dict(gate=gate[1:-1], a2=f["a2"].t, g1=f["g1"].t))
    for n, gt in T.items():
        assert gt.unchanged(), f"input {n} or its guard rows changed"
    for n, gt in o.items():
        assert gt.guards_intact(), f"guard rows of {n} overwritten"
        assert torch.equal(_bits(gt.t), _bits(plain[n])), f"{n}: differs from hdmoe_fusion_out_bwd's"
    tag = f"out rows={rows} dgate={use_dgate}"
    ref = K._out_reference(d, use_dgate)
    diff = float((dal.cpu().double() - plain["dalpha"].cpu().double()).abs())
    bound = 2 * 8 * ULP * float(ref["dalpha"].abs() + ref["dalpha_scale"]) + 2.0 ** -126
    print(f"{tag} dalpha: |wg - plain| {diff:.3e}  bound {bound:.3e}")
    assert diff <= bound, (diff, bound)
    layers = (("out_proj", T["o2"].t, plain["dat"], 32, 32), ("gate1", plain["cat"], plain["dg1"], 64, 32), ("gate2", plain["s"], plain["dl"], 32, 2))
    for g, (name, x, dy, I, O) in zip(G, layers):
        _check_slab(f"{tag} {name}", g, _wgrad_old(call, x.contiguous(), dy.contiguous(), rows, I, O), x, dy)


def test_wg_entry_points_refuse_outside_the_domain(call):
    rows = 40
    d, T, W, sw, _ = K._setup(1, rows, 5)
    big = torch.full((rows * 32 + 8,), FILL, dtype=BF16, device=DEV)
    off = big[4:4 + rows * 32]                                                      # 8 bytes off a 16-byte boundary
    outs = {n: Guarded(rows) for n in ("dfu", "dfv", "do2", "da", "dU")}
    G = [Slab(32, 32), Slab(32, 32), Slab(32, 32), Slab(32, 64), Slab(2, 32)]
    dsw, dal = torch.zeros(1, dtype=F32, device=DEV), torch.zeros(1, dtype=F32, device=DEV)

    def fin(dfu, dtype=1, C=32, r=rows):
        return call("hdmoe_fusion_in_bwd_wg", T["dq"].t, T["dk"].t, T["dv"].t, None, None, T["fu"].t, T["fv"].t, sw, W["wdq"], W["wdk"], W["wdv"],
                    dfu, outs["dfv"].t, dsw, G[0].t, G[1].t, G[2].t, CAP, r, rows, C, 1.0, 1.0, 1.0, dtype)

    assert fin(off) == 1 and fin(outs["dfu"].t, dtype=0) == 1 and fin(outs["dfu"].t, C=64, r=rows // 2) == 1
    d2, T2, W2, dgate, alpha = K._out_setup(rows, 3)
    gate = torch.zeros(rows, 2, dtype=F32, device=DEV)
    a2, g1 = T2["a"].t, T2["U"].t                                                    # (any aligned rows: nothing may be launched)

    def fout(da, dtype=1, C=32):
        return call("hdmoe_fusion_out_bwd_wg", T2["dmixed"].t, None, gate, T2["U"].t, a2, g1, T2["o2"].t, T2["a"].t, alpha, W2["wo"], W2["wdo"],
                    W2["wd1"], W2["wd2"], outs["do2"].t, da, outs["dU"].t, dal, G[0].t, G[3].t, G[4].t, CAP, rows, C, K.AO, K.BO, K.WA, K.WB,
                    1.0, 1.0, dtype)

    assert fout(off) == 1 and fout(outs["da"].t, dtype=0) == 1 and fout(outs["da"].t, C=64) == 1
    torch.cuda.synchronize()
    assert all(o.unchanged() for o in outs.values()) and bool((big == FILL).all()) and float(dsw) == 0.0 and float(dal) == 0.0
    assert all(g.guards_intact() and torch.equal(g.t, g.fill) for g in G)


MID_CASES = [(r, True) for r in ROWS] + [(257, False)]
AQ = K._f32(0.875)                                           # q_proj's output scale (1 in the model; another value shows it is applied)


@pytest.mark.parametrize("rows,slabs", MID_CASES, ids=[f"rows{r}-{'wg' if w else 'nowg'}" for r, w in MID_CASES])
def test_mid_chain_against_the_launches_it_replaces(call, rows, slabs):
    g = torch.Generator().manual_seed(23 * rows + 5)
    T = {n: Guarded(rows, torch.randn(rows, 32, generator=g).to(BF16).to(DEV)) for n in ("o1", "query", "da", "dq2")}
    wo, wq = ((torch.randn(32, 32, generator=g) / 32 ** 0.5).to(BF16).to(DEV) for _ in range(2))
    wdo, wdq = wo.t().contiguous(), wq.t().contiguous()
    new = lambda: torch.empty(rows, 32, dtype=BF16, device=DEV)
    # the unfused launches
    conv = lambda x, w, y, res, al, be: call("hdmoe_conv_fwd", x, w, y, res, al, be, None, 1, 1024, 1, 1, rows, 1, rows, 32, 32, 32, 32, 32, 1, 0,
                                             [1], [1], [0], [0], 1)
    pa, pq2, pdq2x, pdo1, pdres = new(), new(), new(), new(), new()
    conv(T["o1"].t, wo, pa, T["query"].t, K.AO, K.BO)
    conv(pa, wq, pq2, None, AQ, 0.0)
    scratch = torch.zeros(1024, dtype=F32, device=DEV)
    assert call("hdmoe_pw_bwd", pa, T["dq2"].t, wdq, pdq2x, [scratch], None, 1, 1024, 1, rows, 32, 32, AQ, 1) == 0
    pdat = T["da"].t + pdq2x
    assert call("hdmoe_pw_bwd", T["o1"].t, pdat, wdo, pdo1, [scratch], None, 1, 1024, 1, rows, 32, 32, K.AO, 1) == 0
    call("hdmoe_axpby", pdres, pdat, None, K.BO, 0.0, rows * 32, 1)
    # the fused ones
    o = {n: Guarded(rows) for n in ("a", "q2", "do1", "dres")}
    G = [Slab(32, 32), Slab(32, 32)]
    assert call("hdmoe_fusion_mid_fwd", T["o1"].t, T["query"].t, wo, wq, o["a"].t, o["q2"].t, rows, 32, K.AO, K.BO, AQ, 1) == 0
    assert call("hdmoe_fusion_mid_bwd", T["da"].t, T["dq2"].t, o["a"].t, T["o1"].t, wdo, wdq, o["do1"].t, o["dres"].t,
                G[0].t if slabs else None, G[1].t if slabs else None, CAP, rows, 32, K.AO, K.BO, AQ, 1) == 0
    torch.cuda.synchronize()
    for n, gt in T.items():
        assert gt.unchanged(), f"input {n} or its guard rows changed"
    for n, ref in (("a", pa), ("q2", pq2), ("do1", pdo1), ("dres", pdres)):
        assert o[n].guards_intact(), f"guard rows of {n} overwritten"
        assert torch.equal(_bits(o[n].t), _bits(ref)), f"{n}: differs from the unfused launches'"
    if slabs:
        _check_slab(f"mid rows={rows} out_proj", G[0], _wgrad_old(call, T["o1"].t, pdat, rows, 32, 32), T["o1"].t, pdat)
        _check_slab(f"mid rows={rows} q_proj", G[1], _wgrad_old(call, pa, T["dq2"].t, rows, 32, 32), pa, T["dq2"].t)
    else:
        assert all(s.guards_intact() and torch.equal(s.t, s.fill) for s in G)


def test_mid_entry_points_refuse_outside_the_domain(call):
    rows = 40
    T = {n: Guarded(rows, torch.ones(rows, 32, dtype=BF16, device=DEV)) for n in ("o1", "query", "da", "dq2", "a")}
    o = {n: Guarded(rows) for n in ("a", "q2", "do1", "dres")}
    w = torch.zeros(32, 32, dtype=BF16, device=DEV)
    big = torch.full((rows * 32 + 8,), FILL, dtype=BF16, device=DEV)
    off = big[4:4 + rows * 32]                                                      # 8 bytes off a 16-byte boundary
    G = [Slab(32, 32), Slab(32, 32)]
    fwd = lambda a_out, dt=1, C=32: call("hdmoe_fusion_mid_fwd", T["o1"].t, T["query"].t, w, w, a_out, o["q2"].t, rows, C, 1.0, 1.0, 1.0, dt)
    bwd = lambda do1, dt=1, C=32: call("hdmoe_fusion_mid_bwd", T["da"].t, T["dq2"].t, T["a"].t, T["o1"].t, w, w, do1, o["dres"].t, G[0].t, G[1].t,
                                       CAP, rows, C, 1.0, 1.0, 1.0, dt)
    assert fwd(off) == 1 and fwd(o["a"].t, dt=0) == 1 and fwd(o["a"].t, C=64) == 1
    assert bwd(off) == 1 and bwd(o["do1"].t, dt=0) == 1 and bwd(o["do1"].t, C=64) == 1
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in list(T.values()) + list(o.values())) and bool((big == FILL).all())
    assert all(s.guards_intact() and torch.equal(s.t, s.fill) for s in G)


KV_FWD = [(rows, 768) for rows in (1, 31, 32, 33, 257)] + [(33, 512), (33, 1088)]


@pytest.mark.parametrize("rows,Kc", KV_FWD, ids=[f"rows{r}-K{k}" for r, k in KV_FWD])
def test_paired_kv_forward_is_bit_equal_to_two_launches(call, rows, Kc):
    g = torch.Generator().manual_seed(rows * 7 + Kc)
    xb = torch.full((rows + 2 * K.GUARD, Kc), FILL, dtype=BF16, device=DEV)
    x = xb[K.GUARD:K.GUARD + rows]
    x.copy_(torch.randn(rows, Kc, generator=g).to(BF16))
    before = xb.clone()
    w = [(torch.randn(32, Kc, generator=g) / Kc ** 0.5).to(BF16).to(DEV) for _ in range(2)]
    al = (1.0, K._f32(0.75))
    new = [Guarded(rows) for _ in range(2)]
    assert call("hdmoe_kgemm2_fwd", x, w[0], w[1], new[0].t, new[1].t, rows, Kc, al[0], al[1], 1) == 0, "hdmoe_kgemm2_fwd declined a shape of its domain"
    old = [Guarded(rows) for _ in range(2)]
    for i in range(2):
        call("hdmoe_conv_fwd", x, w[i], old[i].t, None, al[i], 0.0, None, 1, w[i].numel(), 1, 1, rows, 1, rows, Kc, Kc, Kc, 32, 32, 1, 0, [1], [1], [0], [0], 1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(xb), _bits(before)), "x or its guard rows changed"
    ref = [al[i] * (x.double() @ w[i].double().t()) for i in range(2)]
    for i, n in enumerate(("k", "v")):
        assert new[i].guards_intact(), f"guard rows of {n} overwritten"
        assert torch.equal(_bits(new[i].t), _bits(old[i].t)), f"{n}: differs from hdmoe_conv_fwd's"
        err = float((new[i].t.double() - ref[i]).abs().max())
        print(f"kv fwd rows={rows} K={Kc} {n}: max|ref| {float(ref[i].abs().max()):.3e}  err {err:.3e}")
        assert bool(((new[i].t.double() - ref[i]).abs() <= 2.0 ** -7 * ref[i].abs() + 1e-5).all()), (n, err)   # a bf16 ulp: the layout is right


KV_BWD = [1, 63, 64, 65, 257, 1000]


@pytest.mark.parametrize("rows", KV_BWD)
def test_paired_kv_weight_gradients(call, rows):
    Kc = 768
    g = torch.Generator().manual_seed(rows * 13 + 1)
    x = torch.randn(rows, Kc, generator=g).to(BF16).to(DEV)
    dy = [Guarded(rows, torch.randn(rows, 32, generator=g).to(BF16).to(DEV)) for _ in range(2)]
    x0 = x.clone()
    G = [Slab(32, Kc), Slab(32, Kc)]
    assert call("hdmoe_lwgrad2", x, dy[0].t, dy[1].t, G[0].t, G[1].t, rows, Kc, 1) == 0, "hdmoe_lwgrad2 declined a shape of its domain"
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(x0)) and dy[0].unchanged() and dy[1].unchanged(), "an input changed"
    for i, n in enumerate(("k_proj", "v_proj")):
        _check_slab(f"kv rows={rows} {n}", G[i], _wgrad_old(call, x, dy[i].t, rows, Kc, 32), x, dy[i].t)


def test_paired_kv_entry_points_refuse_outside_the_domain(call):
    rows, Kc = 40, 768
    big = torch.full((rows * Kc + 8,), FILL, dtype=BF16, device=DEV)
    off = big[4:4 + rows * Kc].view(rows, Kc)                                       # 8 bytes off a 16-byte boundary
    x = torch.zeros(rows, Kc, dtype=BF16, device=DEV)
    w = torch.zeros(32, Kc, dtype=BF16, device=DEV)
    y, dy = [Guarded(rows) for _ in range(2)], [Guarded(rows, torch.ones(rows, 32, dtype=BF16, device=DEV)) for _ in range(2)]
    G = [Slab(32, Kc), Slab(32, Kc)]
    fwd = lambda xx, Kx=Kc, dt=1: call("hdmoe_kgemm2_fwd", xx, w, w, y[0].t, y[1].t, rows, Kx, 1.0, 1.0, dt)
    bwd = lambda xx, Kx=Kc, dt=1: call("hdmoe_lwgrad2", xx, dy[0].t, dy[1].t, G[0].t, G[1].t, rows, Kx, dt)
    assert fwd(off) == 1 and fwd(x, dt=0) == 1 and fwd(x, Kx=256) == 1 and fwd(x, Kx=544) == 1     # misaligned, fp32, below 512, no multiple of 64
    assert bwd(off) == 1 and bwd(x, dt=0) == 1 and bwd(x, Kx=96) == 1
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in y + dy) and bool((big == FILL).all())
    assert all(s.guards_intact() and torch.equal(s.t, s.fill) for s in G)


TAIL_LAYERS = [f"{m}.{l}.weights" for m in ("cross_attn", "cross_attn_text") for l in ("q_proj", "k_proj", "v_proj", "out_proj")] + \
              ["gate1.weights", "gate2.weights"]
# which arguments of an entry point are weight-gradient slabs, and (pointwise launches of one layer) its x and dy
SLAB_ARGS = {"hdmoe_fusion_in_bwd_wg": (14, 15, 16), "hdmoe_fusion_out_bwd_wg": (17, 18, 19), "hdmoe_fusion_mid_bwd": (8, 9), "hdmoe_lwgrad2": (3, 4)}
LAYER_ARGS = {"hdmoe_pw_bwd": 4, "hdmoe_conv_wgrad": 2}      # x, dy = arguments 0, 1; the slab list


def _tail_run(fused_flag):
    """_fusion_tail forward + backward at B = 2 on the wide_config1 weights, twice (the first step registers the layers with the weight
    bank), as tests/test_fusion_stage_kernels.py runs it.  Returns the outputs and gradients of the second step, the names of its C-ABI
    calls, and per tail layer the slab as its launch left it (the bank zeroes the slabs at the start of a step and each layer adds once)
    with -- from a launch that serves one layer -- that layer's x and dy, and the float64 terms of the unfused chain's two fp32 reductions
    (dalpha, dsw per sample), formed from the arguments of their launches."""
    import hdmoe_hip
    from hdmoe_hip import bank as wbank
    from hdmoe_hip import ops
    from conftest import wide_setup
    g = torch.load(os.path.join(ROOT, "tests", "golden", "wide_config1.pt"), weights_only=False)
    hdmoe_hip.set_compute_dtype(BF16)
    old, real = ops.FUSION_FUSED, ops.call
    ops.FUSION_FUSED = fused_flag
    rec = dict(on=False, log=[], slab={}, xy={}, terms={})

    def spy(name, *args):
        rc = real(name, *args)
        if rec["on"]:
            rec["log"].append(name)
            slabs = [args[i] for i in SLAB_ARGS.get(name, ())] + (list(args[LAYER_ARGS[name]]) if name in LAYER_ARGS else [])
            slabs = [t for t in slabs if t is not None]
            if rc == 0 and slabs:
                torch.cuda.synchronize()
                for t in slabs:
                    rec["slab"][t.data_ptr()] = t.detach().clone()
                if name in LAYER_ARGS:
                    x, dy = args[0], args[1]
                    rec["xy"][slabs[0].data_ptr()] = (x.detach().reshape(-1, x.shape[-1]).clone(), dy.detach().reshape(-1, dy.shape[-1]).clone())
            if name == "hdmoe_lerp_param_bwd":                  # (dal_, dat, dalpha, da2, a, at, alpha, n): dalpha = <da2, at - a>
                rec["terms"]["dalpha"] = (args[3].detach().double() * (args[5].detach().double() - args[4].detach().double())).reshape(1, -1)
            if name == "hdmoe_scale_rows_bwd":                  # (dt, dsw, dd, t, sw, B, row length): dsw[n] = <dd[n], t[n]>
                rec["terms"]["dsw"] = (args[2].detach().double() * args[3].detach().double()).reshape(int(args[5]), -1)
        return rc

    ops.call = spy
    try:
        variant, model, kw, state, inp = wide_setup(g)
        model.load_state_dict(state)
        model = model.to(DEV).train()
        net = model.net
        B, R, C = 2, kw["IN_img_resolution"], net.internal_channels
        gen = torch.Generator().manual_seed(11)
        mk = lambda *s: torch.randn(*s, generator=gen).to(DEV)
        out_u, out_v = mk(B, R, R, C).to(BF16).requires_grad_(True), mk(B, R, R, C).to(BF16).requires_grad_(True)
        s_vit, s_unet = (1.0 + 0.1 * mk(B)).requires_grad_(True), (1.0 - 0.1 * mk(B)).requires_grad_(True)
        text = mk(B, 77, kw["text_emb_dim"]).to(BF16)
        gy, ggate = mk(B, R, R, kw["IN_in_channels"]), mk(B, R, R, 2)
        for step in range(2):
            for t in (out_u, out_v, s_vit, s_unet):
                t.grad = None
            model.zero_grad(set_to_none=False)
            rec["on"] = step == 1
            wbank.bank_for(model).begin_step(True)
            try:
                out, gate = net._fusion_tail(out_u, out_v, s_vit, s_unet, text, alpha_routing=10)
            finally:
                wbank.deactivate()
            torch.autograd.backward([out, gate], [gy.to(out.dtype), ggate.to(gate.dtype)])
        torch.cuda.synchronize()
        rec["on"] = False
        res = dict(out=out.detach().float().cpu(), gate=gate.detach().float().cpu(), d_out_u=out_u.grad.float().cpu(), d_out_v=out_v.grad.float().cpu(),
                   d_s_vit=s_vit.grad.float().cpu(), d_s_unet=s_unet.grad.float().cpu())
        names = {id(p): n for n, p in net.named_parameters()}
        for n, p in net.named_parameters():
            if n.split(".")[0] in ("cross_attn", "cross_attn_text", "gate1", "gate2", "alpha_txt") and p.grad is not None:
                res["grad:" + n] = p.grad.detach().float().cpu().clone()
        layers = {}
        for ent in wbank.bank_for(model).entries.values():
            for p, G in zip(ent.params, ent.G):
                n = names.get(id(p))
                if n in TAIL_LAYERS and G.data_ptr() in rec["slab"]:
                    assert n not in layers, f"{n}: two bank entries of one layer were used in the step"
                    layers[n] = (rec["slab"][G.data_ptr()], rec["xy"].get(G.data_ptr()))
        return res, rec["log"], layers, {k: v.cpu() for k, v in rec["terms"].items()}
    finally:
        ops.FUSION_FUSED, ops.call = old, real
        hdmoe_hip.set_compute_dtype(F32)


def test_fusion_tail_in_kernel_weight_gradients_against_the_unfused_ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from hdmoe_hip import ops
    sel0 = ops.kernel_selections()
    fused, step, slabs_f, _ = _tail_run(True)
    sel1 = ops.kernel_selections()
    plain, log_p, slabs_p, terms = _tail_run(False)
    sel2 = ops.kernel_selections()
    assert [sel1[n] - sel0[n] for n in ("fusion_mid", "fusion_mid_bwd")] == [1, 1] and [sel2[n] - sel1[n] for n in ("fusion_mid", "fusion_mid_bwd")] == [0, 0]
    print({n: step.count(n) for n in sorted(set(step)) if "fusion" in n or "wgrad" in n or "pw_bwd" in n})
    assert step.count("hdmoe_fusion_in_fwd") == 1 and step.count("hdmoe_fusion_out_fwd") == 1
    assert step.count("hdmoe_fusion_in_bwd_wg") == 1 and step.count("hdmoe_fusion_out_bwd_wg") == 1
    assert step.count("hdmoe_fusion_in_bwd") == 0 and step.count("hdmoe_fusion_out_bwd") == 0
    assert step.count("hdmoe_kgemm2_fwd") == 1 and step.count("hdmoe_lwgrad2") == 1
    assert step.count("hdmoe_fusion_mid_fwd") == 1 and step.count("hdmoe_fusion_mid_bwd") == 1 and step.count("hdmoe_pw_bwd") == 0
    assert step.count("hdmoe_conv_wgrad") == 1, "a weight-only launch besides output_proj's"
    assert not any(n.endswith("_wg") or "fusion_mid" in n or n in ("hdmoe_kgemm2_fwd", "hdmoe_lwgrad2") for n in log_p)
    assert set(fused) == set(plain) and all("grad:" + n in fused for n in TAIL_LAYERS) and "grad:alpha_txt" in fused
    for n in ("out", "gate", "d_out_u", "d_out_v"):
        assert torch.isfinite(fused[n]).all() and torch.equal(fused[n], plain[n]), f"{n}: the fused stage differs from the unfused ops"
    # The bank's own slabs, as the launches reached through ops.py left them, against the float64 contraction of the unfused run's x and
    # dy (bit-equal to the fused run's: the asserts above, and the kernel tests).  Bound: see the docstring, "Model level".
    assert sorted(slabs_f) == sorted(slabs_p) == sorted(TAIL_LAYERS), (sorted(slabs_f), sorted(slabs_p))
    bad, kappa = [], {}                                          # (every figure is printed before anything is asserted)
    for n in TAIL_LAYERS:
        (Gf, _), (Gp, xy) = slabs_f[n], slabs_p[n]
        x, dy = xy
        ref = (dy.double().t() @ x.double()).reshape(-1)
        mag = (dy.double().abs().t() @ x.double().abs()).reshape(-1)
        assert ref.numel() == Gf.numel() == Gp.numel(), n
        bound = 8 * ULP * (ref.abs() + mag) + 2.0 ** -126
        ef, ep = (Gf.double() - ref).abs(), (Gp.double() - ref).abs()
        kappa[n] = float(mag.max() / ref.abs().max())
        print(f"slab {n}: max|ref| {float(ref.abs().max()):.3e}  kappa {kappa[n]:.1f}  worst err / bound: unfused launch {float((ep / bound).max()):.3f}  "
              f"fused launch {float((ef / bound).max()):.3f}  (max err {float(ep.max()):.3e} / {float(ef.max()):.3e})")
        if not (torch.isfinite(Gf).all() and bool((ef <= bound).all()) and bool((ep <= bound).all())):
            bad.append((n, float(ef.max()), float(ep.max())))
    # what the optimizer sees, fused against unfused
    for n in sorted(fused):
        if n in ("out", "gate", "d_out_u", "d_out_v"):
            continue
        a, b = fused[n].double(), plain[n].double()
        err, scale = (a - b).abs(), float(b.abs().max())
        if n == "grad:alpha_txt":
            t = terms["dalpha"]
            bound = 2 * 8 * ULP * (t.sum(1).abs() + t.abs().sum(1)).reshape(err.shape)
        elif n in ("d_s_vit", "d_s_unet"):
            t = terms["dsw"]
            bound = b.abs() * (2 * 8 * ULP * (t.sum(1).abs() + t.abs().sum(1)) / t.sum(1).abs() + 4 * ULP)
        else:
            bound = torch.full_like(err, 2 * 8 * ULP * (1.0 + kappa[n[5:]]) * scale)
        print(f"{n}: max|unfused| {scale:.3e}  max |fused - unfused| {float(err.max()):.3e}  worst / bound {float((err / bound).max()):.3f}  "
              f"(largest bound {float(bound.max()):.3e})")
        if not (torch.isfinite(a).all() and bool((err <= bound).all())):
            bad.append((n, float(err.max()), float(bound.max())))
    assert not bad, bad
