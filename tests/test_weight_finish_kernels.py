"""The weight prepare and finish kernels against float64 on the CPU, on every code path -- GPU, plus one CPU-only sensitivity test.

hdmoe_wprep_fwd / hdmoe_wbank_prep (before the forward) and hdmoe_wprep_bwd / hdmoe_wbank_bwd (after the backward) stand between every
conv / linear kernel and the optimiser.  The entry points are called directly (hdmoe_hip._lib.call), the bank descriptors are built from
hdmoe_hip.bank._DESC, the reference is fp64 on the CPU from the same fp32 operands, and the bounds are elementwise.

Reference of the two backward kernels, per output row o (fan = I kh kw, weight element e = i * taps + t, g_e = G[t][o][i]):
    c = fan^-1/2,  n = ||w_o||,  dd = 1e-4 + n c,  s = gain c,  k1 = out_scale s / dd,  kap = out_scale s c / (dd^2 n)  (0 when n == 0)
    dw_e = pre_e + k1 g_e - kap (sum_j w_j g_j) w_e                 (normalize == 0: dw_e = pre_e + out_scale g_e)
pre = what the gradient buffer held (hdmoe_wbank_bwd accumulates; hdmoe_wprep_bwd overwrites: pre = 0, out_scale = 1).
Bound per element, with T_e = |pre_e| + |k1| |g_e| + |w_e| kap sum_j |w_j g_j| and M = ceil(fan / 128) + 16:
    |got - ref| <= K M 2^-24 T_e,   K = 2;   T_e == 0: exact.
K is derived, not tuned: a 128-thread strided sum followed by the block tree passes through at most ceil(fan / 128) + 8 roundings, the
error of the sum of squares reaches k2 with factor 1.5 (dd^2 n), and the scalar chain adds about a dozen roundings.  A plain fp32
evaluation of the same formulas on the CPU (sequential sums) against fp64 needed K <= 0.30 over fan 2 .. 6400 with the data kinds below.
Each case's needed K of the kernel goes to build/measurements/weight_finish.json (with the worst); K is not tightened from them.

Data kinds, as separate rows of every tensor (a one-row tensor takes one kind, rotating): random rows with a per-row scale 0.2 .. 2.2;
an all-zero row; a row with g = 1.7 w + 1e-3 noise (the two terms nearly cancel); a row scaled by 1e-5 (n c below the 1e-4 epsilon);
a row scaled by 1e3.

Which case reaches which path of wbank_bwd_kernel (csrc/wbank.hip; by the shape alone: staged when taps > 1 and taps (I + 1) <= 2560):
    staged through LDS   (2,3,3) fewer elements than threads; (32,3,3); (283,3,3) 9 * 284 = 2556, the last staged 3x3; (101,5,5) 2550;
                         (639,2,2) exactly 2560; (7,1,3) non-square
    direct, taps == 1    (36,1,1), (129,1,1), (768,1,1)
    direct, large rows   (284,3,3) 2565; (102,5,5) 2575; (640,2,2) 2564; (64,7,7)
each with O in {1, 17} (one tensor O = 33), normalize in {1, 0}, out_scale in {1, fp32(0.6)}, gain 1.75, all in ONE launch; three of them
also alone; and under row lists (rows 5 .. O - 1 only, a tensor absent, shuffled order) as bank.py finish_stage / _finish build them.
wprep_bwd_kernel (csrc/conv.hip) has one path per normalize; (G, O, I, ks) = (1,17,36,[1]), (3,5,32,[3,5,7]), (8,2,6,[3,3,3,5,5,5,7,7])
(HDMOE_MAX_GROUPS) and (1,3,768,[1]), with and without per-group gain scalars and dgain accumulators.
wprep_fwd_kernel: fp32 / bf16 / split images x normalize x mutate x flip x (wd or none) x (gain scalars or none), G = 3 groups of kernel
sizes 3, 5, 1 inside one 25-tap stride.
"""
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "build", "measurements")     # measured errors (kept out of git: build/)
DEV = "cuda"
U = 2.0 ** -24
K = 2.0                                                   # see the module docstring: derived, not tuned
K_CPU_FP32 = 0.30                                         # what a sequential fp32 evaluation on the CPU needs (for the record in the JSON)
GAIN = 1.75                                               # exact in fp32
SCALE_06 = float(torch.tensor(0.6, dtype=torch.float32))  # the fp32 value the descriptor carries
# hi + lo of a split-bf16 image against fp64, relative.  bf16 keeps 8 significant bits, so for the fp32 value v with 2^e <= |v| < 2^(e+1):
# |v - hi| <= 2^(e-8) (half an ulp; NOT 2^-9 |v|: at the bottom of a binade that is 2^-8 |v|), r = v - hi is exact in fp32, and either
# |r| = 2^(e-8), a bf16 number (lo exact), or r lies in a binade <= e - 9 and |r - lo| <= 2^(e-17).  So |v - hi - lo| <= 2^-17 |v|, and it is
# attained (test_split_bound_derivation).  v itself is the fp32 image's value, within 4 * 2^-24 of the reference: in all
# 2^-17 (1 + 4 * 2^-24) + 4 * 2^-24 = 1.031 * 2^-17.  (First stated as 2^-17: 2^-18 for the split from the 2^-9 above, plus the fp32
# term, rounded up; an MI355X measured 1.002 * 2^-17 at O = 32, I = 36, k = 5 with the fp32 image at 3.35 * 2^-24 -- the kernel rounds to
# nearest twice, which is the best two bf16 numbers can do, so the derivation was corrected, not the kernel.)
SPLIT_REL = 2.0 ** -17 * (1.0 + 4.0 * U) + 4.0 * U
MARGIN = 64                                               # sentinel floats on either side of a gradient buffer
SENTINEL = -12345.0
KINDS = ("rand", "zero", "cancel", "tiny", "huge")

STAGED = [(2, 3, 3), (32, 3, 3), (283, 3, 3), (101, 5, 5), (639, 2, 2), (7, 1, 3)]
DIRECT_1 = [(36, 1, 1), (129, 1, 1), (768, 1, 1)]
DIRECT_L = [(284, 3, 3), (102, 5, 5), (640, 2, 2), (64, 7, 7)]

_measured = {}


def bank_path(I, kh, kw):
    """The path of wbank_bwd_kernel a shape takes (csrc/wbank.hip: WB_LDS_FLOATS = 2560)."""
    taps = kh * kw
    if taps > 1 and taps * (I + 1) <= 2560:
        return "staged"
    return "direct-1" if taps == 1 else "direct-large"


def make_rows(O, fan, gen, kinds=None):
    """(w, g): (O, fan) fp32 rows of the data kinds, row r of kind kinds[r] (random past the end of the list)."""
    kinds = list(KINDS if kinds is None else kinds)
    w = torch.randn(O, fan, generator=gen) * (0.2 + 2.0 * torch.rand(O, 1, generator=gen))
    g = torch.randn(O, fan, generator=gen)
    for r, kind in enumerate(kinds[:O]):
        if kind == "zero":
            w[r] = 0.0
        elif kind == "cancel":
            g[r] = 1.7 * w[r] + 1e-3 * torch.randn(fan, generator=gen)
        elif kind == "tiny":
            w[r] *= 1e-5
        elif kind == "huge":
            w[r] *= 1e3
    return w.float().contiguous(), g.float().contiguous()


def finish_ref(w, g, pre, gain, out_scale, normalize):
    """fp64 reference and magnitude of the finish kernels.  w, g, pre: (O, fan) float64 in weight order -> (ref, T, contribution)."""
    fan = w.shape[1]
    if not normalize:
        con = out_scale * g
        return pre + con, pre.abs() + abs(out_scale) * g.abs(), con
    c = fan ** -0.5
    n = w.norm(dim=1, keepdim=True)
    dd = 1e-4 + n * c
    s = gain * c
    k1 = out_scale * s / dd
    kap = torch.where(n > 0, out_scale * s * c / (dd * dd * n.clamp_min(1e-300)), torch.zeros_like(n))
    gw = (w * g).sum(dim=1, keepdim=True)
    agw = (w * g).abs().sum(dim=1, keepdim=True)
    con = k1 * g - kap * gw * w
    T = pre.abs() + k1.abs() * g.abs() + w.abs() * kap.abs() * agw
    return pre + con, T, con


def needed_k(got, ref, T, fan):
    """The smallest K for which |got - ref| <= K M 2^-24 T holds at every element (inf: a non-finite result, or T = 0 and not exact)."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    d = (got - ref).abs()
    if bool(((T == 0) & (d > 0)).any()):
        return float("inf")
    if d.numel() == 0:
        return 0.0
    M = math.ceil(fan / 128) + 16
    return float((d / (M * U * torch.where(T > 0, T, torch.ones_like(T)))).max())


def to_slab(g, I, taps):
    """(O, fan) in weight order e = i * taps + t  ->  the [tap][O][I] slab."""
    return g.view(g.shape[0], I, taps).permute(2, 0, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- CPU only
def test_bound_rejects_injected_faults():
    """The bound function applied to the fp64 reference itself, at (32,3,3), O = 17, all data kinds: the correct result rounded to fp32
    passes; each injected fault is rejected."""
    I, taps, O = 32, 9, 17
    fan = I * taps
    gen = torch.Generator().manual_seed(6)
    w32, g32 = make_rows(O, fan, gen)
    pre32 = torch.randn(O, fan, generator=gen)
    w, g, pre = w32.double(), g32.double(), pre32.double()
    zero = KINDS.index("zero")

    for scale in (1.0, SCALE_06):
        for normalize in (1, 0):
            ref, T, _ = finish_ref(w, g, pre, GAIN, scale, normalize)
            assert needed_k(ref.float(), ref, T, fan) <= K
    ref, T, con = finish_ref(w, g, pre, GAIN, SCALE_06, 1)

    def rejected(bad):
        return not needed_k(bad.float(), ref, T, fan) <= K

    c = fan ** -0.5
    n = w.norm(dim=1, keepdim=True)
    dd = 1e-4 + n * c
    k1 = SCALE_06 * GAIN * c / dd
    kap = torch.where(n > 0, SCALE_06 * GAIN * c * c / (dd * dd * n.clamp_min(1e-300)), torch.zeros_like(n))
    gw = (w * g).sum(dim=1, keepdim=True)
    # 1. the k2 term dropped
    assert rejected(pre + k1 * g)
    # 2. c applied once instead of twice in k2
    assert rejected(pre + k1 * g - (kap / c) * gw * w)
    # 3. out_scale dropped
    assert rejected(finish_ref(w, g, pre, GAIN, 1.0, 1)[0])
    assert not needed_k(finish_ref(w, g, pre, GAIN, 1.0, 0)[0].float(), *finish_ref(w, g, pre, GAIN, SCALE_06, 0)[:2], fan) <= K
    # 4. '=' instead of '+=' into a non-zero gradient
    assert rejected(con)
    # 5. tap and input-channel indices swapped in the slab read: element e decoded as (t, i) = (e / I, e % I) instead of (e % taps, e / taps)
    slab = to_slab(g, I, taps)                                           # [t][o][i]
    e = torch.arange(fan)
    g_bad = slab[e // I, :, e % I].transpose(0, 1)                       # (O, fan)
    assert not torch.equal(g_bad, g)
    assert rejected(finish_ref(w, g_bad, pre, GAIN, SCALE_06, 1)[0])
    # 6. one row's contribution written to the neighbouring row
    bad = ref.clone()
    bad[7], bad[8] = pre[7], pre[8] + con[8] + con[7]
    assert rejected(bad)
    bad = ref.clone()
    bad[[7, 8]] = pre[[7, 8]] + con[[8, 7]]
    assert rejected(bad)
    # 7. the all-zero row treated with dd = n c: inf or NaN
    bad = ref.clone()
    with_zero_dd = (SCALE_06 * GAIN * c / (n[zero] * c)) * g[zero]
    bad[zero] = pre[zero] + with_zero_dd - (SCALE_06 * GAIN * c * c * gw[zero] / ((n[zero] * c) ** 2 * n[zero])) * w[zero]
    assert not bool(torch.isfinite(bad[zero]).all())
    assert rejected(bad)
    # and a wrong k2 on the one small-norm row alone (what a max-relative check over the tensor lets through)
    tiny = KINDS.index("tiny")
    bad = ref.clone()
    bad[tiny] = pre[tiny] + k1[tiny] * g[tiny]
    assert rejected(bad)


def test_split_bound_derivation():
    """The split term of SPLIT_REL on the CPU: rounding to nearest twice leaves at most 2^-17 |v|, and more than 2^-18 |v| at some values
    (bottom of a binade, r just past a bf16 rounding midpoint) -- so no bound below 2^-17 can hold for a correct kernel."""
    gen = torch.Generator().manual_seed(4)
    v = torch.cat([torch.randn(1 << 20, generator=gen), 1.0 + torch.rand(1 << 20, generator=gen) / 64.0])
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    rel = float((((v.double() - hi.double()) - lo.double()).abs() / v.double().abs()).max())
    assert 2.0 ** -18 < rel <= 2.0 ** -17, rel
    assert 2.0 ** -17 < SPLIT_REL < 1.04 * 2.0 ** -17


def test_every_bank_path_has_a_case():
    assert {bank_path(*s) for s in STAGED} == {"staged"}
    assert {bank_path(*s) for s in DIRECT_1} == {"direct-1"}
    assert {bank_path(*s) for s in DIRECT_L} == {"direct-large"}
    assert 4 * (639 + 1) == 2560 and 9 * (283 + 1) == 2556 and 9 * (284 + 1) == 2565


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.fixture(scope="module")
def call():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    yield call
    if _measured:
        os.makedirs(OUT_DIR, exist_ok=True)
        with open(os.path.join(OUT_DIR, "weight_finish.json"), "w") as f:
            json.dump(dict(cases=_measured, worst=max(_measured.values()), bound=dict(K=K), cpu_fp32_needed_K=K_CPU_FP32), f, indent=1, sort_keys=True)


def _note(tag, k):
    _measured[tag] = max(_measured.get(tag, 0.0), k)


# ---- 1. hdmoe_wbank_bwd
def _bank_specs():
    specs = []
    for I, kh, kw in STAGED + DIRECT_1 + DIRECT_L:
        for O in (1, 17):
            for normalize in (1, 0):
                for scale in (1.0, SCALE_06):
                    specs.append((I, kh, kw, O, normalize, scale))
    specs.append((32, 3, 3, 33, 1, SCALE_06))
    return specs


def _bank_build(specs, seed):
    """Descriptors and operands of one hdmoe_wbank_bwd launch: per tensor a record with the device buffers and the fp64 operands."""
    import numpy as np
    from hdmoe_hip.bank import _DESC
    gen = torch.Generator().manual_seed(seed)
    descs = np.zeros(len(specs), dtype=_DESC)
    recs = []
    for di, (I, kh, kw, O, normalize, scale) in enumerate(specs):
        taps = kh * kw
        fan = I * taps
        w, g = make_rows(O, fan, gen, None if O > 1 else [KINDS[di % len(KINDS)]])
        pre = torch.randn(O, fan, generator=gen)
        slab = to_slab(g, I, taps)
        buf = torch.full((MARGIN + O * fan + MARGIN,), SENTINEL)
        buf[MARGIN:MARGIN + O * fan] = pre.reshape(-1)
        r = dict(spec=specs[di], fan=fan, taps=taps, w_cpu=w, slab_cpu=slab, pre_cpu=pre, buf_cpu=buf.clone(),
                 w=w.to(DEV), slab=slab.to(DEV), buf=buf.to(DEV), w64=w.double(), g64=g.double(), pre64=pre.double(),
                 tag=f"bank ({I},{kh},{kw}) O={O} norm={normalize} scale={scale:.1f} [{bank_path(I, kh, kw)}]")
        d = descs[di]
        d["w_raw"], d["G"], d["dw"] = r["w"].data_ptr(), r["slab"].data_ptr(), r["buf"].data_ptr() + 4 * MARGIN
        d["O"], d["I"], d["kh"], d["kw"], d["Ipad"], d["Opad"] = O, I, kh, kw, (I + 15) // 16 * 16, (O + 15) // 16 * 16
        d["normalize"], d["mutate_ok"], d["gain"], d["out_scale"] = normalize, 1, GAIN, scale
        recs.append(r)
    return torch.from_numpy(descs.view(np.uint8).copy()).to(DEV), recs


def _bank_launch(call, dd, rows):
    rr = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).contiguous().to(DEV)
    call("hdmoe_wbank_bwd", dd, rr, len(rows))
    torch.cuda.synchronize()


def _bank_check(r, listed, launches, suffix=""):
    """One tensor after `launches` identical launches over its rows `listed`: operands and margins untouched, unlisted rows bit-identical
    to pre, listed rows pre + launches * contribution within launches * the bound.  Returns the needed K (of one launch's bound)."""
    I, kh, kw, O, normalize, scale = r["spec"]
    fan, tag = r["fan"], r["tag"] + suffix
    assert torch.equal(r["w"].cpu().view(torch.int32), r["w_cpu"].view(torch.int32)), f"{tag}: w_raw changed"
    assert torch.equal(r["slab"].cpu().view(torch.int32), r["slab_cpu"].view(torch.int32)), f"{tag}: the slab changed"
    buf = r["buf"].cpu()
    assert torch.equal(buf[:MARGIN], r["buf_cpu"][:MARGIN]) and torch.equal(buf[-MARGIN:], r["buf_cpu"][-MARGIN:]), f"{tag}: margins written"
    got = buf[MARGIN:-MARGIN].view(O, fan)
    listed = sorted(listed)
    unlisted = [o for o in range(O) if o not in set(listed)]
    assert torch.equal(got[unlisted].view(torch.int32), r["pre_cpu"][unlisted].view(torch.int32)), f"{tag}: an unlisted row was written"
    if not listed:
        return 0.0
    _, T, con = finish_ref(r["w64"], r["g64"], r["pre64"], GAIN, scale, normalize)
    ref = r["pre64"] + launches * con
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite gradient"
    k = needed_k(got[listed], ref[listed], T[listed], fan) / launches
    print(f"{tag}: needed K = {k:.4f}")
    assert k <= K, f"{tag}: needed K = {k:.3f} > {K}"
    # the all-zero rows: pre + k1 g with dd = 1e-4 exactly, no projection term
    zr = [o for o in listed if not bool(r["w64"][o].any())]
    if zr and normalize:
        k1 = scale * GAIN * fan ** -0.5 / 1e-4
        zref = r["pre64"][zr] + launches * k1 * r["g64"][zr]
        zT = r["pre64"][zr].abs() + abs(k1) * r["g64"][zr].abs()
        kz = needed_k(got[zr], zref, zT, fan) / launches
        assert kz <= K, f"{tag}: all-zero row: needed K = {kz:.3f}"
    return k


@pytest.mark.gpu
def test_bank_finish_every_path_in_one_launch(call):
    """Every (shape, O, normalize, out_scale) tensor of the module docstring's table in ONE launch, into non-zero gradients between sentinel
    margins; then the same launch again (accumulation across backward passes): pre + 2 * the contribution within twice the bound."""
    specs = _bank_specs()
    assert {bank_path(*s[:3]) for s in specs} == {"staged", "direct-1", "direct-large"}
    dd, recs = _bank_build(specs, 101)
    rows = [(di, o) for di, r in enumerate(recs) for o in range(r["spec"][3])]
    _bank_launch(call, dd, rows)
    for r in recs:
        _note(r["tag"], _bank_check(r, range(r["spec"][3]), 1))
    _bank_launch(call, dd, rows)
    for r in recs:
        _note(r["tag"] + " twice", _bank_check(r, range(r["spec"][3]), 2, " (second launch)"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(283, 3, 3), (768, 1, 1), (284, 3, 3)], ids=["staged", "direct-1", "direct-large"])
def test_bank_finish_one_descriptor_alone(call, shape):
    dd, recs = _bank_build([shape + (17, 1, SCALE_06)], 202 + shape[0])
    _bank_launch(call, dd, [(0, o) for o in range(17)])
    _note(recs[0]["tag"] + " alone", _bank_check(recs[0], range(17), 1, " (alone)"))


@pytest.mark.gpu
def test_bank_finish_row_lists(call):
    """The subset launches of bank.py finish_stage and the `rest` branch of _finish: one tensor lists only its rows 5 .. O - 1, one tensor
    is absent, and the (descriptor, row) pairs come in a shuffled order.  Unlisted rows keep their bits; listed rows hold the bound."""
    specs = [s for s in _bank_specs() if s[3] > 1 and s[5] != 1.0]
    dd, recs = _bank_build(specs, 303)
    partial = next(i for i, s in enumerate(specs) if s[:3] == (283, 3, 3) and s[4] == 1)
    absent = next(i for i, s in enumerate(specs) if s[:3] == (284, 3, 3) and s[4] == 1)
    listed = {di: list(range(5 if di == partial else 0, s[3])) for di, s in enumerate(specs) if di != absent}
    rows = [(di, o) for di, os_ in listed.items() for o in os_]
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(9)).tolist()
    rows = [rows[p] for p in perm]
    assert rows != sorted(rows)
    _bank_launch(call, dd, rows)
    for di, r in enumerate(recs):
        _note(r["tag"] + " row list", _bank_check(r, listed.get(di, []), 1, " (row list)"))


# ---- 2. hdmoe_wprep_bwd
PREP_BWD_CASES = [(1, 17, 36, [1]), (3, 5, 32, [3, 5, 7]), (8, 2, 6, [3, 3, 3, 5, 5, 5, 7, 7]), (1, 3, 768, [1])]
GAIN_SCALARS = [0.5, 1.25, 0.8125, 1.5, 0.75, 2.0, 0.625, 1.125]          # distinct, exact in fp32


def _prep_bwd_operands(G, O, I, ks, seed):
    gen = torch.Generator().manual_seed(seed)
    ops_ = []
    for g_, k in enumerate(ks):
        fan = I * k * k
        kinds = [KINDS[(g_ + r) % len(KINDS)] for r in range(O)] if O < len(KINDS) else None
        w, g = make_rows(O, fan, gen, kinds)
        ops_.append((w, g, to_slab(g, I, k * k)))
    return ops_


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [1, 0], ids=["norm", "plain"])
@pytest.mark.parametrize("G,O,I,ks", PREP_BWD_CASES, ids=["1x17x36", "3x5x32", "8x2x6", "1x3x768"])
def test_prep_bwd_matches_fp64(call, G, O, I, ks, normalize):
    """hdmoe_wprep_bwd (argument order as ops._conv_wgrad calls it) into NaN-filled gradients: every element written (overwrite
    semantics) and within the bound; normalize == 0: the relaid-out slab bit for bit; the learnable-gain gradient
    dgain_g = pre_g + sum_o gain_val c gw_o / dd_o within 2 (M + O) 2^-24 (|pre_g| + sum_o gain_val c / dd_o sum_e |w_e g_e|) -- the + O
    for the order of the atomic adds over the rows."""
    ops_ = _prep_bwd_operands(G, O, I, ks, 400 + G + O + I)
    for with_gain in (False, True):
        for with_dgain in (False, True):
            tag = f"prep_bwd {(G, O, I)} norm={normalize} gain={int(with_gain)} dgain={int(with_dgain)}"
            ws = [w.view(O, I, k, k).to(DEV) for (w, _, _), k in zip(ops_, ks)]
            slabs = [s.to(DEV) for _, _, s in ops_]
            dws = [torch.full_like(w, float("nan")) for w in ws]
            gains = [torch.tensor(GAIN_SCALARS[g_], device=DEV) for g_ in range(G)] if with_gain else None
            dg_pre = [0.3 + 0.7 * g_ for g_ in range(G)]
            dgs = [torch.tensor(v, dtype=torch.float32, device=DEV) for v in dg_pre] if with_dgain else None
            call("hdmoe_wprep_bwd", ws, gains, GAIN, slabs, dws, dgs, ks, ks, G, O, I, normalize)
            torch.cuda.synchronize()
            worst = 0.0
            for g_, k in enumerate(ks):
                w32, g32, slab = ops_[g_]
                fan = I * k * k
                assert torch.equal(ws[g_].cpu().view(O, fan), w32) and torch.equal(slabs[g_].cpu(), slab), f"{tag} group {g_}: operands changed"
                got = dws[g_].cpu().view(O, fan)
                assert bool(torch.isfinite(got).all()), f"{tag} group {g_}: an element was not written"
                if not normalize:
                    assert torch.equal(got.view(torch.int32), g32.view(torch.int32)), f"{tag} group {g_}: not the relaid-out slab"
                    if with_dgain:
                        assert float(dgs[g_]) == float(torch.tensor(dg_pre[g_], dtype=torch.float32)), f"{tag} group {g_}: dgain touched"
                    continue
                w, g = w32.double(), g32.double()
                gain = GAIN * (float(torch.tensor(GAIN_SCALARS[g_], dtype=torch.float32)) if with_gain else 1.0)
                ref, T, _ = finish_ref(w, g, torch.zeros_like(w), gain, 1.0, 1)
                kk = needed_k(got, ref, T, fan)
                worst = max(worst, kk)
                assert kk <= K, f"{tag} group {g_} (k = {k}): needed K = {kk:.3f} > {K}"
                if with_dgain:
                    c = fan ** -0.5
                    dd = 1e-4 + w.norm(dim=1) * c
                    pre = float(torch.tensor(dg_pre[g_], dtype=torch.float32))
                    dref = pre + float((GAIN * c * (w * g).sum(dim=1) / dd).sum())
                    dT = abs(pre) + float((GAIN * c * (w * g).abs().sum(dim=1) / dd).sum())
                    M = math.ceil(fan / 128) + 16
                    dk = abs(float(dgs[g_]) - dref) / ((M + O) * U * dT)
                    print(f"{tag} group {g_}: dgain needed K = {dk:.4f}")
                    _note(tag + " dgain", dk)
                    assert dk <= K, f"{tag} group {g_}: dgain {float(dgs[g_])} vs {dref}: needed K = {dk:.3f} > {K}"
            if normalize:
                print(f"{tag}: needed K = {worst:.4f}")
                _note(tag, worst)


@pytest.mark.gpu
def test_prep_bwd_refuses_bad_group_counts(call):
    """ngroups 0 and 9 (HDMOE_MAX_GROUPS + 1): HDMOE_EINVAL and nothing launched -- the outputs stay NaN."""
    O, I = 2, 6
    gen = torch.Generator().manual_seed(5)
    ws = [torch.randn(O, I, 1, 1, generator=gen).to(DEV) for _ in range(9)]
    slabs = [torch.randn(1, O, I, generator=gen).to(DEV) for _ in range(9)]
    dws = [torch.full_like(w, float("nan")) for w in ws]
    dgs = [torch.full((), float("nan"), device=DEV) for _ in range(9)]
    for n in (0, 9):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call("hdmoe_wprep_bwd", ws, None, GAIN, slabs, dws, dgs, [1] * 9, [1] * 9, n, O, I, 1)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(d).all()) for d in dws + dgs)


# ---- 3. / 4. hdmoe_wprep_fwd and the split lo plane
FWD_DTYPES = {"fp32": (0, torch.float32, torch.int32), "bf16": (1, torch.bfloat16, torch.int16), "split": (2, torch.bfloat16, torch.int16)}
FWD_KS = [3, 5, 1]
FWD_TAPS = 25                                             # the group stride of both images: the largest kernel's taps
FWD_KINDS = ("rand", "zero", "tiny", "huge")


def _pad16(c):
    return (c + 15) // 16 * 16


def _bf16_ulp(r):
    return torch.exp2(torch.floor(torch.log2(r.abs().clamp_min(1e-300))) - 7.0)


def _prep_fwd_case(call, dt, normalize, mutate, flip, with_wd, with_gain, O, I, seed):
    code, idt, bits = FWD_DTYPES[dt]
    planes = 2 if dt == "split" else 1
    G = len(FWD_KS)
    Ipad, Opad = _pad16(I), _pad16(O)
    gen = torch.Generator().manual_seed(seed)
    w0s = [make_rows(O, I * k * k, gen, FWD_KINDS)[0] for k in FWD_KS]
    ws = [w.view(O, I, k, k).to(DEV) for w, k in zip(w0s, FWD_KS)]
    gvals = [float(torch.tensor(v, dtype=torch.float32)) for v in GAIN_SCALARS[:G]]
    gains = [torch.tensor(v, device=DEV) for v in gvals] if with_gain else None
    wstride, wdstride = FWD_TAPS * O * Ipad, FWD_TAPS * I * Opad
    wf = torch.full((planes * G * wstride,), float("nan"), dtype=idt, device=DEV)
    wd = torch.full((planes * G * wdstride,), float("nan"), dtype=idt, device=DEV) if with_wd else None
    call("hdmoe_wprep_fwd", ws, gains, GAIN, FWD_KS, FWD_KS, G, O, I, Ipad, Opad, wf, wstride, wd, wdstride, normalize, mutate, flip, code)
    torch.cuda.synchronize()
    tag0 = f"prep_fwd {dt} O={O} I={I} norm={normalize} mutate={mutate} flip={flip} wd={int(with_wd)} gain={int(with_gain)}"
    F = wf.view(planes, G, FWD_TAPS, O, Ipad).cpu()
    B = wd.view(planes, G, FWD_TAPS, I, Opad).cpu() if with_wd else None
    worst = worst_lo = 0.0
    for g_, k in enumerate(FWD_KS):
        tag = f"{tag0} group {g_} (k = {k})"
        taps = k * k
        fan = I * taps
        f = F[:, g_]
        # unused taps keep the sentinel; the pad columns of the used taps are zero in every plane
        assert bool(torch.isnan(f[:, taps:]).all()), f"{tag}: taps past k^2 of the forward image written"
        assert not bool(f[:, :taps, :, I:].contiguous().view(bits).any()), f"{tag}: pad columns I .. Ipad not zero"
        assert bool(torch.isfinite(f[:, :taps, :, :I]).all()), f"{tag}: an element of the forward image was not written"
        if with_wd:
            b = B[:, g_]
            assert bool(torch.isnan(b[:, taps:]).all()), f"{tag}: taps past k^2 of the flipped image written"
            assert not bool(b[:, :taps, :, O:].contiguous().view(bits).any()), f"{tag}: pad rows O .. Opad of wd not zero"
            bt = b[:, :taps].flip(1) if flip else b[:, :taps]
            assert torch.equal(f[:, :taps, :, :I].contiguous().view(bits), bt[:, :, :, :O].transpose(2, 3).contiguous().view(bits)), \
                f"{tag}: wd does not carry the bits of wf (flip = {flip})"
        # values
        w0 = w0s[g_].double()
        stored = ws[g_].cpu().view(O, fan)
        c = fan ** -0.5
        ref = w0
        if normalize:
            gain = GAIN * (gvals[g_] if with_gain else 1.0)
            inv = 1.0 / (1e-4 + w0.norm(dim=1, keepdim=True) * c)
            if mutate:
                want_n, got_n = (w0 * inv).norm(dim=1), stored.double().norm(dim=1)
                assert bool(((got_n - want_n).abs() <= 1e-6 * want_n).all()), f"{tag}: norm of the mutated rows"
                wm = stored.double()                              # the forward's weight is the normalisation of the parameter AS STORED
                inv = 1.0 / (1e-4 + wm.norm(dim=1, keepdim=True) * c)
                ref = wm * inv * gain * c
            else:
                ref = w0 * inv * gain * c
        if not (normalize and mutate):
            assert torch.equal(stored.view(torch.int32), w0s[g_].view(torch.int32)), f"{tag}: w_raw changed"
        ref = ref.view(O, I, taps).permute(2, 0, 1)               # [tap][o][i]
        hi = f[0, :taps, :, :I].double()
        if dt == "fp32":
            ratio = float(((hi - ref).abs() / (4.0 * U * ref.abs()).clamp_min(1e-300)).max())
        else:
            ratio = float(((hi - ref).abs() / _bf16_ulp(ref)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
        if dt == "split":
            lo = f[1, :taps, :, :I].double()
            r_lo = float(((hi + lo - ref).abs() / (SPLIT_REL * ref.abs()).clamp_min(1e-300)).max())
            worst_lo = max(worst_lo, r_lo)
            assert r_lo <= 1.0, f"{tag}: |hi + lo - ref| / (SPLIT_REL |ref|) = {r_lo:.3f}"
    return worst, worst_lo


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [1, 0], ids=["norm", "plain"])
@pytest.mark.parametrize("dt", list(FWD_DTYPES))
def test_prep_fwd_images(call, dt, normalize):
    """hdmoe_wprep_fwd (argument order as _MPConvFn.forward calls it) into NaN-filled images, G = 3 groups with k = 3, 5, 1 in one 25-tap
    stride, over mutate x flip x (wd | none) x (gain scalars | none): the first k^2 taps of each group match the fp64 normalisation (of the
    rows as stored, when the prepare mutates) to 4 * 2^-24 relative (fp32) or one bf16 ulp (bf16, hi plane of split); hi + lo of split to
    SPLIT_REL = 1.031 * 2^-17 relative (derived at the constant); columns I .. Ipad (both planes) and rows O .. Opad of wd are zero; wd carries wf's bits at [taps-1-t][i][o] (flip) or
    [t][i][o]; w_raw keeps its bits unless normalize and mutate.  Taps k^2 .. 24 of a smaller group KEEP THE SENTINEL: the kernel never
    writes them, which is the contract ops.py's torch.empty images rely on (no conv kernel reads a group's taps past its own k^2)."""
    shapes = [(16, 6), (32, 36)] if dt == "split" else [(5, 6), (17, 36)]
    worst = worst_lo = 0.0
    for O, I in shapes:
        for mutate in (0, 1):
            for flip in (1, 0):
                for with_wd in (True, False):
                    for with_gain in (False, True):
                        a, b = _prep_fwd_case(call, dt, normalize, mutate, flip, with_wd, with_gain, O, I, 500 + O + I)
                        worst, worst_lo = max(worst, a), max(worst_lo, b)
    print(f"prep_fwd {dt} normalize={normalize}: worst |err| / bound = {worst:.3f}, split hi + lo: {worst_lo:.3f}")


@pytest.mark.gpu
def test_prep_fwd_return_codes(call):
    O, I = 16, 6
    w = torch.randn(O, I, 3, 3).to(DEV)

    def run(Ipad=16, Opad=16, code=0, with_wd=True, idt=torch.float32, planes=1):
        wf = torch.full((planes * 9 * O * 16,), float("nan"), dtype=idt, device=DEV)
        wd = torch.full((planes * 9 * I * 32,), float("nan"), dtype=idt, device=DEV) if with_wd else None
        try:
            call("hdmoe_wprep_fwd", [w], None, GAIN, [3], [3], 1, O, I, Ipad, Opad, wf, 9 * O * 16, wd, 9 * I * 32, 1, 0, 1, code)
        finally:
            torch.cuda.synchronize()
            assert bool(torch.isnan(wf).all()) and (wd is None or bool(torch.isnan(wd).all())), "a refused call wrote an image"

    with pytest.raises(RuntimeError, match="invalid argument"):
        run(Ipad=8)                                           # Ipad % 16 != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        run(Ipad=0)                                           # Ipad < I
    with pytest.raises(RuntimeError, match="invalid argument"):
        run(Ipad=4)                                           # both
    with pytest.raises(RuntimeError, match="invalid argument"):
        run(Opad=32, code=2, idt=torch.bfloat16, planes=2)    # split with wd and Opad != O
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        run(code=7)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        run(code=3)                                           # (fp16 is hdmoe_cast's only)


# ---- 5. one check through the bank
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["plain", "bank"])
def test_two_backward_passes_accumulate_through_mp_conv(call, path):
    """An fp32 layer N = 3, 8 x 8, 8 -> 8, k = 3 through ops.mp_conv: without a bank (hdmoe_wprep_fwd / hdmoe_wprep_bwd) and with a bank
    prepared by begin_step(True), the mutating prepare (hdmoe_wbank_prep / hdmoe_wbank_bwd; the bank serves a layer from the step after
    it first saw it: one warm-up step).  Two backward passes without clearing .grad.  Each train-mode prepare re-normalises the stored
    parameter (w / (1e-4 + 1) on an already normalised row), so each pass's fp64 autograd gradient of MP_Conv is evaluated on the values
    stored after THAT pass's prepare and the two are summed -- "twice the gradient", exactly.  Each path against fp64, not one another."""
    import hdmoe_hip._lib as L
    from hdmoe_hip import ops, bank as wbank
    from oracle import hdmoe_oracle as Orc
    gen = torch.Generator().manual_seed(55)
    x = torch.randn(3, 8, 8, 8, generator=gen)                # NHWC
    gy = torch.randn(3, 8, 8, 8, generator=gen)
    w0 = torch.randn(8, 8, 3, 3, generator=gen)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(w0.clone())
    m = M().to(DEV)
    xd, gd = x.to(DEV), gy.to(DEV)

    def step():
        if path == "bank":
            wbank.bank_for(m).begin_step(True)
        xx = xd.clone().requires_grad_(True)
        y = ops.mp_conv(xx, m.w, 0.9, training=True)
        stored = m.w.detach().cpu().double()                  # as stored after this pass's prepare
        y.backward(gd)
        wbank.deactivate()
        torch.cuda.synchronize()
        return stored

    def fp64_grad(stored):
        w64 = stored.clone().requires_grad_(True)
        Orc.mp_conv(x.permute(0, 3, 1, 2).double(), w64, 0.9).backward(gy.permute(0, 3, 1, 2).double())
        return w64.grad

    wbank.deactivate()
    saved_log = L.CALL_LOG
    try:
        if path == "bank":
            step()                                            # warm-up: registers the layer
            m.w.grad = None
        L.CALL_LOG = []
        ref = fp64_grad(step())
        once = m.w.grad.detach().cpu().double().clone()
        ref2 = ref + fp64_grad(step())
        names = [n for n, _ in L.CALL_LOG]
    finally:
        L.CALL_LOG = saved_log
        wbank.deactivate()
    if path == "bank":
        assert names.count("hdmoe_wbank_prep") == 2 and names.count("hdmoe_wbank_bwd") == 2 and "hdmoe_wprep_bwd" not in names, names
    else:
        assert names.count("hdmoe_wprep_fwd") == 2 and names.count("hdmoe_wprep_bwd") == 2 and "hdmoe_wbank_bwd" not in names, names
    twice = m.w.grad.detach().cpu().double()
    for got, want, what in ((once, ref, "one pass"), (twice, ref2, "two passes")):
        err, lim = float((got - want).abs().max()), 1e-4 * float(want.abs().max()) + 1e-6
        print(f"mp_conv {path} {what}: max|dw - fp64| = {err:.3e} (limit {lim:.3e})")
        assert err <= lim, f"{path}, {what}: max|dw - fp64| = {err:.3e} > {lim:.3e}"
