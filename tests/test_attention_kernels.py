"""The dense attention kernels of csrc/attention.hip against float64 on the CPU, on every path hdmoe_attn_fwd / hdmoe_attn_bwd can launch.

Reference.  Operands are drawn from a seed and rounded to the case's dtype; the same values are evaluated in float64 (`_formula`):
s = q k^T / sqrt(D) (+ bias[:, :Sq, :Skv]), lse = logsumexp(s), p = exp(s - lse), out = p v, and with dP = dO v^T, delta = dO . out:
dS = p (dP - delta), dv = p^T dO, dq = dS k / sqrt(D), dk = dS^T q / sqrt(D), dbias = sum_b dS.  `_calibrate` asserts that these
formulas are torch's float64 autograd gradients of the same forward.  A direct hdmoe_attn_bwd call gets `out` and `lse` of the
reference rounded to their storage types, and the reference's delta uses that same rounded `out`; the ops.attention tests hand
the formulas the `out` the kernel itself saved.

Bounds, per element, never per tensor.  u = 2**-24.  An output element k with reference r must satisfy
    generic kernels   |k - r| <= K u (|r| + A S)                          (+ 2**-8 |r| when the output is stored as bf16)
    MFMA kernels      |k - r| <= K_M (u |r| + 2**-8 S + 2**-16 A S)       (+ 2**-8 |r|)
with S the sum of the magnitudes of the terms the element is made of,
    out    sum_j p |v|                                 dq     scale sum_j p (|dP| + |delta|) |k|
    lse    1 + |lse|                                   dk     scale sum_i p (|dP| + |delta|) |q|
    dv     sum_i p |dO|                                dbias  sum_b p (|dP| + |delta|)      (+ |pre-fill| when dbias accumulates)
and A = 1 + max|s| + max|lse| over the (sample, head) pair: what an fp32 rounding of the exponent's argument does to p (for dbias the
sum over the samples takes each sample's own A).  The MFMA unit comes from the kernel header: probabilities and dS are rounded to bf16
before the second product and the denominator is summed from the rounded probabilities (2**-8 S); c q is carried as a hi + lo bf16
pair, -lse as a 2-term and -delta as a 3-term bf16 expansion (2**-16 A S).
Zero and non-finite patterns: wherever the reference is non-finite the kernel must be; wherever an element has no non-zero term
(S = 0) the kernel must give an exact zero, and so must out, lse and dv wherever the reference is exactly zero.  An exact zero of dq,
dk or dbias with S > 0 is the cancellation dP - delta (Skv = 1), which the MFMA kernels evaluate as a bf16 expansion: those elements
are held to the bound.  No element is ever excluded.
Underflow.  The large-score rows have probabilities below the range of fp32 (e**-1000), where the relative bound above cannot be met
by any fp32 or bf16 kernel: the hardware exp flushes a result under TINY = 2**-126 (the smallest normal number of both formats) to zero,
and so do the product p dP and the store of the output.  Every bound therefore carries the absolute term TINY (1 + the same sum with
p = 1 and |dP| + |delta| + 1 in place of |dP| + |delta|); it is 1e-38 times sums of operand magnitudes and does not take part in K.

K is four times the worst ratio |fp32 CPU - fp64| / (u (|r| + A S)) that `_calibrate` measured with `_formula` in float32 over every
case table of this file, rounded up to a power of two (the kernels sum in another order and use fast exp).  K_M is four times the
worst ratio of `_emulate` -- float64 with exactly the roundings named above, with the first-tile shift and with the row maximum --
against the MFMA unit, over the MFMA tables.  Run as `PYTHONPATH=. python tests/test_attention_kernels.py`; never by a test.
  quantity   worst fp32-CPU ratio (case)                          4 x worst    K     worst emulation ratio (case)          4 x worst   K_M
  out          1.09  (D = 32 fp32, Sq 255, Skv 17)                     4.36      8     0.761 (Sq 257, Skv 5, H 1)               3.05      4
  lse          0.78  (D = 32 fp32, Sq 1, Skv 1)                        3.14      4     0.401 (Sq 255, Skv 1, H 8)               1.60      2
  dq          71.93  (D = 32 fp32, Sq 255, Skv 1: dP - delta cancels  287.7    512     0.674 (B 600, Sq 40, Skv 33, H 8)        2.70      4
                      and the 32-term dot products behind |dP| and
                      |delta| are summed in different orders)
  dk          19.35  (D = 32 fp32, Sq 1, Skv 127)                     77.4     128     0.942 (Sq 1, Skv 160, H 8)               3.77      4
  dv           1.35  (D = 32 fp32, Sq 1, Skv 15)                       5.40      8     0.928 (Sq 1, Skv 160, H 8)               3.71      4
  dbias        6.00  (D = 32 fp32, B 2, Sq 257, Skv 129, Sb 257)      24.0      32
  dtable       1.19  (test_wrapper_bias_from_bicubic_resize)           4.77      8
On the MI355X the kernels' own worst |error| / bound came out, for fp32 outputs of the generic kernels, at 0.16 (out), 0.17 (lse), 0.03 (dq),
0.44 (dk), 0.25 (dv), 0.62 (dbias) and 0.11 (dtable); with bf16 outputs the rounding of the store (2**-8 |r|) is most of the bound and the
worst ratios are 0.93 ... 1.00.  MFMA kernels: 0.23 (out), 0.20 (lse), 0.27 (dq), 0.29 (dk), 0.30 (dv).  Each test prints its own.

Which kernel ran.  Every case asserts from the difference in ops.kernel_selections() that the launch its table names was the one
enqueued: attn_fwd_mfma, attn_bwd_merged (Sq <= 1024), attn_bwd_pair (Sq > 1024) or attn_generic (one count per call).
"""
import math
import os
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
TINY = 2.0 ** -126                                                  # smallest normal fp32 / bf16 number
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
KEYS = ("out", "lse", "dq", "dk", "dv", "dbias")
K = dict(out=8.0, lse=4.0, dq=512.0, dk=128.0, dv=8.0, dbias=32.0, dtable=8.0)      # generic kernels (the table of the module docstring)
KM = dict(out=4.0, lse=2.0, dq=4.0, dk=4.0, dv=4.0)                                  # MFMA kernels
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
PAD = 64                                                            # sentinel elements on either side of every output
FWD_MFMA, BWD_MERGED, BWD_PAIR, GENERIC = "attn_fwd_mfma", "attn_bwd_merged", "attn_bwd_pair", "attn_generic"

# Sb = 0: no bias.  sq / sk scale q / k; first: k[:, :32] *= first (the MFMA forward's shift comes from the first 32 keys);
# dead16: k[:, :16] *= 0.01 (the row maximum is not in the generic forward's first chunk of 16)
Case = namedtuple("Case", "B Sq Skv H D dt Sb sq sk first dead16", defaults=(4, "bf16", 0, 1.0, 1.0, None, False))


def _id(c):
    s = f"B{c.B}-Sq{c.Sq}-Skv{c.Skv}-H{c.H}-D{c.D}-{c.dt}"
    s += f"-Sb{c.Sb}" if c.Sb else ""
    s += f"-x{c.sq:g}x{c.sk:g}" if (c.sq, c.sk) != (1.0, 1.0) else ""
    s += f"-first{c.first:g}" if c.first is not None else ""
    return s + ("-dead16" if c.dead16 else "")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    return call


def _ops():
    from hdmoe_hip import ops
    return ops


# =====================================================================================================
# reference
# =====================================================================================================
def _heads(t, H):
    B, S, E = t.shape
    return t.view(B, S, H, E // H).transpose(1, 2)              # (B, H, S, D)


def _flat(t):
    B, H, S, D = t.shape
    return t.transpose(1, 2).reshape(B, S, H * D)


@lru_cache(maxsize=2)
def _inputs(c):
    """q, k, v, dO (and the bias table) of a case as float64 CPU tensors that hold values of the case's dtype (the table: fp32)."""
    g = torch.Generator(device="cpu").manual_seed(((c.B * 1009 + c.Sq) * 1013 + c.Skv) * 1019 + c.H * 37 + c.D)
    E, dt = c.H * c.D, DT[c.dt]
    q = c.sq * torch.randn(c.B, c.Sq, E, generator=g)
    k = c.sk * torch.randn(c.B, c.Skv, E, generator=g)
    if c.first is not None:
        k[:, :32] *= c.first
    if c.dead16:
        k[:, :16] *= 0.01
    v = torch.randn(c.B, c.Skv, E, generator=g)
    go = torch.randn(c.B, c.Sq, E, generator=g)
    bias = (0.5 * torch.randn(c.H, c.Sb, c.Sb, generator=g)).double() if c.Sb else None
    q, k, v, go = (t.to(dt).double() for t in (q, k, v, go))
    return dict(q=q, k=k, v=v, go=go, bias=bias)


def _over_batch(fn, inp, H, **kw):
    """fn over slices of the batch (at most 2**22 scores at a time), results concatenated; the dbias entries are summed."""
    B, Sq, Skv = inp["q"].shape[0], inp["q"].shape[1], inp["k"].shape[1]
    nb = max(1, (1 << 22) // (H * Sq * Skv))
    parts = []
    for b0 in range(0, B, nb):
        sl = slice(b0, b0 + nb)
        sub = {n: (t[sl] if (t is not None and n != "bias") else t) for n, t in inp.items()}
        parts.append(fn(sub, H, **{n: (t[sl] if torch.is_tensor(t) else t) for n, t in kw.items()}))
    res = {}
    for grp in parts[0]:
        res[grp] = {}
        for key in parts[0][grp]:
            vals = [p[grp][key] for p in parts]
            res[grp][key] = sum(vals[1:], vals[0]) if key == "dbias" else torch.cat(vals, 0)
    return res


def _formula_slice(inp, H, ft=torch.float64, out_in=None, round_out=None, scales=True):
    q, k, v, go = (_heads(inp[n].to(ft), H) for n in ("q", "k", "v", "go"))
    Sq, Skv, D = q.shape[2], k.shape[2], q.shape[3]
    scale = 1.0 / math.sqrt(D)
    s = (q @ k.transpose(-1, -2)) * scale
    if inp["bias"] is not None:
        s = s + inp["bias"][:, :Sq, :Skv].to(ft)
    lse = torch.logsumexp(s, -1)
    p = (s - lse[..., None]).exp()
    out = p @ v
    if out_in is not None:                                       # the `out` the backward kernel is given
        used = _heads(out_in.to(ft), H)
    elif round_out is not None:
        used = out.to(round_out).to(ft)
    else:
        used = out
    delta = (go * used).sum(-1)
    dP = go @ v.transpose(-1, -2)
    dS = p * (dP - delta[..., None])
    r = dict(out=_flat(out), lse=lse, dq=_flat(dS @ k * scale), dk=_flat(dS.transpose(-1, -2) @ q * scale), dv=_flat(p.transpose(-1, -2) @ go))
    if inp["bias"] is not None:
        r["dbias"] = dS.sum(0)
    res = dict(r={n: t.double() for n, t in r.items()}, aux=dict(out_in=_flat(used).double()))
    if scales:
        A = 1.0 + s.abs().amax((-1, -2)) + lse.abs().amax(-1)    # (B, H)
        A4 = A[:, :, None, None]
        m = p * (dP.abs() + delta.abs()[..., None])
        S = dict(out=_flat(p @ v.abs()), lse=1.0 + lse.abs(), dq=_flat(m @ k.abs() * scale), dk=_flat(m.transpose(-1, -2) @ q.abs() * scale),
                 dv=_flat(p.transpose(-1, -2) @ go.abs()))
        AS = dict(out=_flat(A4 * (p @ v.abs())), lse=A[:, :, None] * S["lse"], dq=_flat(A4 * (m @ k.abs()) * scale),
                  dk=_flat(A4 * (m.transpose(-1, -2) @ q.abs()) * scale), dv=_flat(A4 * (p.transpose(-1, -2) @ go.abs())))
        one = torch.ones_like(p)                                 # the same sums with p = 1 and a flush of dS itself: what TINY multiplies
        m1 = 1.0 + dP.abs() + delta.abs()[..., None]
        F = dict(out=_flat(1.0 + one @ v.abs()), lse=torch.zeros_like(lse), dq=_flat(1.0 + m1 @ k.abs() * scale),
                 dk=_flat(1.0 + m1.transpose(-1, -2) @ q.abs() * scale), dv=_flat(1.0 + one.transpose(-1, -2) @ go.abs()))
        if inp["bias"] is not None:
            S["dbias"], AS["dbias"], F["dbias"] = m.sum(0), (A4 * m).sum(0), m1.sum(0)
        res["S"], res["AS"], res["F"] = S, AS, {n: TINY * t for n, t in F.items()}
    return res


def _formula(inp, H, **kw):
    return _over_batch(_formula_slice, inp, H, **kw)


@lru_cache(maxsize=2)
def _truth(c):
    """float64 reference of a case with `out` rounded to the case's dtype for the backward: r, S, AS = A S and F = the underflow term (dicts by quantity),
    aux.out_in."""
    return _formula(_inputs(c), c.H, round_out=DT[c.dt])


def _bound(t, key, dtype, mfma, extra=0.0):
    a, S, AS = t["r"][key].abs(), t["S"][key] + extra, t["AS"][key] + extra
    b = KM[key] * (U * a + 2.0 ** -8 * S + 2.0 ** -16 * AS) if mfma else K[key] * U * (a + AS)
    return b + t["F"][key] + (2.0 ** -8 * a if dtype == torch.bfloat16 else 0.0)


def _match(k, r, bound, S, msg, zeros):
    """k (device) vs r (fp64 CPU): the same NaN and +-inf positions, an exact zero wherever S is zero (and, zeros=True, wherever r is),
    |k - r| <= bound everywhere else."""
    k = k.detach().cpu().double()
    assert k.shape == r.shape, (msg, k.shape, r.shape)
    assert torch.equal(k.isnan(), r.isnan()), f"{msg}: NaN pattern {int(k.isnan().sum())} vs {int(r.isnan().sum())}"
    assert torch.equal(k.isinf(), r.isinf()) and torch.equal(k[k.isinf()], r[r.isinf()]), f"{msg}: inf pattern"
    exact = (S.expand_as(r) == 0) | ((r == 0) if zeros else torch.zeros_like(r, dtype=torch.bool))
    assert bool((k[exact] == 0).all()), f"{msg}: {int((k[exact] != 0).sum())} non-zeros where the reference has no non-zero term"
    fin = torch.isfinite(r)
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(r)
    err = (k - r).abs()
    bad = fin & (err > b)
    live = fin & (b > 0)
    worst = float((err[live] / b[live]).max()) if live.any() else 0.0
    print(f"{msg}: worst |err| / bound = {worst:.3f}")
    assert not bool(bad.any()), f"{msg}: {int(bad.sum())} entries over the bound, worst |err| {float(err[bad].max()):.3e} " \
                          f"at bound {float(b[bad][err[bad].argmax()]):.3e} (ratio {float((err[bad] / b[bad].clamp_min(1e-300)).max()):.2f})"


def _check(got, t, key, dtype, mfma, tag, extra=0.0, want=None):
    r = t["r"][key] if want is None else want
    tt = t if want is None else dict(t, r=dict(t["r"], **{key: want}))
    _match(got, r, _bound(tt, key, dtype, mfma, extra), t["S"][key] + extra, f"{tag} [{'mfma' if mfma else 'generic'} {str(dtype)[6:]}] {key}",
           zeros=key in ("out", "lse", "dv"))


# =====================================================================================================
# device buffers with sentinel margins, launches with the selection counters read around them
# =====================================================================================================
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Buf:
    """A tensor in the middle of a NaN-filled buffer, PAD elements on either side; off = 1 starts the view one element later, which for
    bf16 leaves it 2-byte aligned (the MFMA launchers want 8)."""

    def __init__(self, shape, dtype, src=None, off=0):
        n = math.prod(shape)
        self.base = torch.full((n + 2 * PAD + off,), float("nan"), dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.base[self.lo:self.hi].view(shape)
        if src is not None:
            self.t.copy_(src.to(dtype))
        assert self.t.is_contiguous() and (self.t.data_ptr() % 8 == 0) == (off == 0 or dtype != torch.bfloat16)

    def margins_kept(self):
        fresh = torch.full_like(self.base, float("nan"))
        return torch.equal(_bits(self.base[:self.lo]), _bits(fresh[:self.lo])) and torch.equal(_bits(self.base[self.hi:]), _bits(fresh[self.hi:]))


def _launched(before):
    after = _ops().kernel_selections()
    return {n: after[n] - before[n] for n in after if after[n] != before[n]}


def _code(c):
    return 0 if c.dt == "fp32" else 1


def _run_fwd(lib, c, off=0):
    inp, dt, E = _inputs(c), DT[c.dt], c.H * c.D
    q, k, v = (Buf(inp[n].shape, dt, inp[n], off).t for n in ("q", "k", "v"))
    bias = inp["bias"].float().to(DEV) if c.Sb else None
    out, lse = Buf((c.B, c.Sq, E), dt, off=off), Buf((c.B, c.H, c.Sq), torch.float32)
    before = _ops().kernel_selections()
    lib("hdmoe_attn_fwd", out.t, lse.t, q, k, v, bias, c.B, c.Sq, c.Skv, c.H, c.D, c.Sb, _code(c))
    torch.cuda.synchronize()
    return out, lse, _launched(before)


def _fwd_case(lib, c, path, off=0, tag=""):
    t, mfma = _truth(c), path != GENERIC
    out, lse, ran = _run_fwd(lib, c, off)
    assert ran == {path: 1}, f"{_id(c)}: launched {ran}, the table says {path}"
    _check(out.t, t, "out", DT[c.dt], mfma, tag + _id(c))
    _check(lse.t, t, "lse", torch.float32, mfma, tag + _id(c))
    assert out.margins_kept() and lse.margins_kept(), "a forward kernel wrote outside out / lse"


def _run_bwd(lib, c, off=0, prefill=None):
    """hdmoe_attn_bwd on the reference's rounded out / lse.  dbias: a NaN-filled [H][Sb][Sb] table whose [:, :Sq, :Skv] corner holds
    `prefill` (zeros if None)."""
    inp, t, dt, E = _inputs(c), _truth(c), DT[c.dt], c.H * c.D
    q, k, v, go = (Buf(inp[n].shape, dt, inp[n], off).t for n in ("q", "k", "v", "go"))
    out = Buf((c.B, c.Sq, E), dt, t["aux"]["out_in"], off).t
    lse = t["r"]["lse"].float().to(DEV)
    dq, dk, dv = Buf((c.B, c.Sq, E), dt, off=off), Buf((c.B, c.Skv, E), dt, off=off), Buf((c.B, c.Skv, E), dt, off=off)
    delta = torch.empty(c.B, c.H, c.Sq, device=DEV)
    bias = dbias = None
    if c.Sb:
        bias = inp["bias"].float().to(DEV)
        dbias = Buf((c.H, c.Sb, c.Sb), torch.float32)
        dbias.t[:, :c.Sq, :c.Skv] = 0.0 if prefill is None else prefill.to(DEV)
        dbias.before = dbias.t.clone()
    before = _ops().kernel_selections()
    lib("hdmoe_attn_bwd", dq.t, dk.t, dv.t, None if dbias is None else dbias.t, delta, go, out, q, k, v, lse, bias, c.B, c.Sq, c.Skv, c.H, c.D,
        c.Sb, _code(c))
    torch.cuda.synchronize()
    return dq, dk, dv, dbias, _launched(before)


def _bwd_case(lib, c, path, off=0, prefill=None, tag=""):
    t, mfma, dt = _truth(c), path != GENERIC, DT[c.dt]
    dq, dk, dv, dbias, ran = _run_bwd(lib, c, off, prefill)
    assert ran == {path: 1}, f"{_id(c)}: launched {ran}, the table says {path}"
    for key, b in (("dq", dq), ("dk", dk), ("dv", dv)):
        _check(b.t, t, key, dt, mfma, tag + _id(c))
        assert b.margins_kept(), f"a backward kernel wrote outside {key}"
    if dbias is not None:
        pre = torch.zeros_like(t["r"]["dbias"]) if prefill is None else prefill.double()
        _check(dbias.t[:, :c.Sq, :c.Skv], t, "dbias", torch.float32, False, tag + _id(c), extra=pre.abs(), want=pre + t["r"]["dbias"])
        outside = torch.ones(c.H, c.Sb, c.Sb, dtype=torch.bool, device=DEV)
        outside[:, :c.Sq, :c.Skv] = False
        assert torch.equal(_bits(dbias.t)[outside], _bits(dbias.before)[outside]), "dbias changed outside [:, :Sq, :Skv]"
        assert dbias.margins_kept(), "a backward kernel wrote outside dbias"


# =====================================================================================================
# 1. MFMA forward (bf16, D = 4, no bias), with the first-tile shift and forced onto the online maximum
# =====================================================================================================
MFMA_FWD = [
    Case(1, 1, 1, 1),                        # one query, one key: wave 0 holds one query, waves 1-7 none; first tile of one key
    Case(2, 31, 5, 2),                       # last wave partly filled; first tile shorter than 32; two stages (even)
    Case(1, 32, 31, 3),                      # a wave exactly full; 31 keys; three stages (odd)
    Case(1, 33, 32, 1),                      # one query in the second wave; one full tile, no remainder; a single stage
    Case(2, 255, 33, 2),                     # the eighth wave one query short; one key in the second tile
    Case(1, 256, 127, 3),                    # a full query block; four tiles through the remainder loop, the last partial
    Case(1, 257, 128, 2),                    # a second query block of one query; exactly one four-tile pointer step
    Case(1, 33, 129, 8),                     # the pointer step, then one key in the remainder loop; eight stages
    Case(2, 31, 160, 3),                     # the pointer step, then one full remainder tile
    Case(1, 33, 1023, 2),                    # seven pointer steps and a remainder that ends one key short of the image
    Case(1, 32, 1024, 3),                    # the whole staged image
    Case(1, 31, 1025, 2),                    # two key chunks (the second holds one key): the online maximum, four stages
    Case(1, 257, 2049, 1),                   # three key chunks, two query blocks, one head (three stages)
    Case(1, 33, 2049, 3),                    # three key chunks x three heads: nine stages
    Case(1, 1, 160, 8),                      # one query against a pointer step
    Case(1, 255, 1, 8),                      # one key: p = 1 for every query
    Case(1, 257, 5, 1),                      # the second query block with a short first tile
    Case(2, 256, 256, 8, sq=6.0, sk=6.0),                    # |s| in the hundreds
    Case(2, 128, 256, 8, sq=8.0, sk=30.0, first=1e-3),       # a later key beats the first-tile shift by more than 2^127: the wave repeats
    Case(2, 128, 256, 8, sq=8.0, sk=0.05, first=600.0),      # the first tile dominates everything after it
]


@pytest.mark.parametrize("c", MFMA_FWD, ids=_id)
def test_mfma_forward(lib, c):
    try:
        for slow in ("0", "1"):
            os.environ["HDMOE_ATTN_SLOW"] = slow
            _fwd_case(lib, c, FWD_MFMA, tag=f"slow={slow} ")
    finally:
        os.environ.pop("HDMOE_ATTN_SLOW", None)


# =====================================================================================================
# 2. merged backward (Sq <= 1024): hg = min(H, ceil(512 / B)) head groups, hpw = ceil(H / hg) heads per workgroup
# =====================================================================================================
MERGED = [Case(B, 40, Skv, H) for Skv in (33, 77) for B, H in [      # Skv = 33 / 77: two / three key passes per head; with three the
    (1, 8),                                  # hpw 1: baseline                      # `parity` of the dK | dV exchange enters the second head at 1
    (128, 8),                                # hpw 2: a second head in the loop
    (256, 8),                                # hpw 4: the benchmark's geometry
    (256, 3),                                # hpw 2: the last workgroup breaks at h = 3
    (200, 5),                                # hpw 2 (hg = 3): the last workgroup breaks at h = 5
    (600, 8)]]                               # hpw 8: one workgroup per sample
MERGED += [Case(2, Sq, 40, 2) for Sq in (    # query-tile ownership (wave w owns tiles 8 w .. 8 w + 7), hpw 1
    1, 33,                                   # wave 0 alone: one query; two tiles
    256,                                     # wave 0 exactly full
    257, 289,                                # wave 1 with one and with two tiles
    1000, 1024)]                             # all four waves: the last tile partial; the whole image
MERGED += [Case(2, 96, Skv, 2) for Skv in (1, 31, 64, 1100)]   # one key (dP - delta cancels); a partial pass; two full passes; 35 passes
MERGED += [Case(2, 256, 256, 8, sq=6.0, sk=6.0), Case(2, 128, 256, 8, sq=8.0, sk=30.0, first=1e-3),
           Case(2, 128, 256, 8, sq=8.0, sk=0.05, first=600.0)]     # the forward's three large-score rows (hpw 1)


@pytest.mark.parametrize("c", MERGED, ids=_id)
def test_merged_backward(lib, c):
    hg = min(c.H, -(-512 // c.B))
    print(f"hpw = {-(-c.H // hg)}")
    _bwd_case(lib, c, BWD_MERGED)


# =====================================================================================================
# 3. dq + dk / dv pair (Sq > 1024): nb32 = ceil(Skv / 32) key blocks, nkb = 8 (nb32 >= 5), 4 (>= 3), else nb32 per workgroup
# =====================================================================================================
PAIR = [
    Case(1, 1025, 20, 1),                    # nkb 1: the queries split eight ways; the second query chunk holds one query
    Case(1, 1056, 20, 3),
    Case(2, 1056, 40, 3),                    # nkb 2: four ways
    Case(1, 1025, 77, 3),                    # nkb 4 with three key blocks: two ways, one block idle
    Case(1, 1056, 77, 1),
    Case(1, 1056, 129, 1),                   # nkb 8, no split; one key in the last block
    Case(1, 1025, 129, 3),
    Case(1, 1025, 1024, 1),                  # four workgroups of eight key blocks
    Case(1, 1056, 1024, 3),
]


@pytest.mark.parametrize("c", PAIR, ids=_id)
def test_pair_backward(lib, c):
    _bwd_case(lib, c, BWD_PAIR)


# =====================================================================================================
# 4. bf16 D = 4 operands without bias that the MFMA launchers refuse: the generic kernels, held to the generic bf16 bound
# =====================================================================================================
MISALIGNED = [Case(2, 40, 33, 8), Case(2, 257, 40, 2), Case(1, 96, 1100, 2), Case(1, 1025, 77, 3), Case(1, 31, 5, 2)]
MANY_HEADS = Case(1, 4, 4, 4097)             # H > 4096


@pytest.mark.parametrize("c", MISALIGNED, ids=_id)
def test_fallback_on_2_byte_aligned_views(lib, c):
    _fwd_case(lib, c, GENERIC, off=1)
    _bwd_case(lib, c, GENERIC, off=1)


def test_fallback_above_4096_heads(lib):
    _fwd_case(lib, MANY_HEADS, GENERIC)
    _bwd_case(lib, MANY_HEADS, GENERIC)


# =====================================================================================================
# 5. generic kernels: TQ = 256 rows per block, TK = 128 rows per LDS tile, online-softmax chunks of CH = 16
# =====================================================================================================
def _generic_cases():
    cs = []
    for D in (1, 2, 4, 8, 16, 32):
        for dt in ("fp32", "bf16"):
            for B, Sq, Skv, H in ((2, 257, 129, 3), (3, 17, 145, 2)):   # a second query block / key tile of one row; 145 = 128 + 16 + 1
                if not (dt == "bf16" and D == 4):                        # (bf16 D = 4 without bias: section 4)
                    cs.append(Case(B, Sq, Skv, H, D, dt))
                for Sb in (max(Sq, Skv), max(Sq, Skv) + 3):              # Sq != Skv under a bias; a table larger than the corner read
                    cs.append(Case(B, Sq, Skv, H, D, dt, Sb))
    for D in (4, 32):                        # tile edges: one row; a block one short / full; chunks of 15, 16, 17 keys; a tile of 127, 128
        for Sq in (1, 255, 256):
            for Skv in (1, 15, 16, 17, 127, 128):
                cs.append(Case(2, Sq, Skv, 2, D, "fp32"))                                   # BIAS = false
                cs.append(Case(2, Sq, Skv, 2, D, "bf16", max(Sq, Skv) + (3 if Skv % 2 else 0)))   # BIAS = true
        for dt in ("fp32", "bf16"):          # |s| in the hundreds, the row maximum past the first chunk of 16
            cs.append(Case(2, 40, 50, 2, D, dt, 0 if dt == "fp32" else 53, sq=6.0, sk=6.0, dead16=True))
    cs += [Case(B, 33, 20, 2, 8, "fp32", 36) for B in (1, 5)]            # the dbias walk over one and five samples
    return cs


GENERIC_CASES = _generic_cases()


@pytest.mark.parametrize("c", GENERIC_CASES, ids=_id)
def test_generic_kernels(lib, c):
    _fwd_case(lib, c, GENERIC)
    _bwd_case(lib, c, GENERIC)


# =====================================================================================================
# 6. repeatability, dbias accumulation, the ops.attention wrapper, refusals
# =====================================================================================================
def test_same_call_same_bits(lib):
    """No float atomics in the dense kernels: a repeated call gives the same bits, one case per path."""
    c = MFMA_FWD[13]
    a, b = _run_fwd(lib, c), _run_fwd(lib, c)
    assert a[2] == b[2] == {FWD_MFMA: 1}
    assert all(torch.equal(_bits(x.t), _bits(y.t)) for x, y in zip(a[:2], b[:2])), "MFMA forward"
    for c, path in ((Case(256, 40, 77, 8), BWD_MERGED), (Case(2, 1056, 40, 3), BWD_PAIR), (Case(2, 257, 129, 3, 8, "bf16", 260), GENERIC)):
        a, b = _run_bwd(lib, c), _run_bwd(lib, c)
        assert a[4] == b[4] == {path: 1}
        for x, y in zip(a[:4], b[:4]):
            assert x is None or torch.equal(_bits(x.t), _bits(y.t)), path
    c = Case(2, 257, 129, 3, 8, "bf16", 260)
    a, b = _run_fwd(lib, c), _run_fwd(lib, c)
    assert a[2] == b[2] == {GENERIC: 1}
    assert all(torch.equal(_bits(x.t), _bits(y.t)) for x, y in zip(a[:2], b[:2])), "generic forward"


@pytest.mark.parametrize("c", [Case(3, 17, 145, 2, 8, "fp32", 148), Case(5, 33, 20, 2, 4, "bf16", 33)], ids=_id)
def test_dbias_accumulates_into_a_filled_table(lib, c):
    """hdmoe_attn_bwd adds to what dbias[:, :Sq, :Skv] holds."""
    g = torch.Generator(device="cpu").manual_seed(11)
    prefill = (torch.randn(c.H, c.Sq, c.Skv, generator=g) + 2.0).float()
    _bwd_case(lib, c, GENERIC, prefill=prefill, tag="pre-filled ")


def _pad_corner(t, Sb):
    full = torch.zeros(t.shape[0], Sb, Sb, dtype=t.dtype)
    full[:, :t.shape[1], :t.shape[2]] = t
    return full


def _wrapper_truth(c, inp, out):
    """The reference with the gradients' delta taken from the `out` the kernel saved; dbias entries padded to the whole table."""
    t = _formula(inp, c.H, out_in=out.detach().cpu().double())
    if c.Sb:
        for grp in ("r", "S", "AS", "F"):
            t[grp]["dbias"] = _pad_corner(t[grp]["dbias"], c.Sb)
    return t


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_wrapper_bias_gradient_modes(lib, dt):
    """ops.attention with the bias gradient fresh (leaf without .grad), accumulating into a non-zero .grad (the kernel adds straight into
    it; a second backward without zero_grad doubles the contribution) and with a bias that needs no gradient."""
    ops = _ops()
    c = Case(3, 40, 33, 2, 8, dt, 43)
    inp, dtype = _inputs(c), DT[dt]
    g = torch.Generator(device="cpu").manual_seed(9)
    for mode in ("fresh", "accumulate", "none"):
        tag = f"ops.attention bias {mode} "
        qd, kd, vd = (inp[n].to(DEV).to(dtype).requires_grad_(True) for n in ("q", "k", "v"))
        bd = inp["bias"].float().to(DEV).requires_grad_(mode != "none")
        base = (torch.randn(c.H, c.Sb, c.Sb, generator=g) + 2.0).float() if mode == "accumulate" else torch.zeros(c.H, c.Sb, c.Sb)
        if mode == "accumulate":
            bd.grad = base.to(DEV).clone()
        for rep in (1, 2) if mode == "accumulate" else (1,):
            for x in (qd, kd, vd):
                x.grad = None
            before = ops.kernel_selections()
            out = ops.attention(qd, kd, vd, bd, c.H)
            out.backward(inp["go"].to(DEV).to(dtype))
            torch.cuda.synchronize()
            assert _launched(before) == {GENERIC: 2}
            t = _wrapper_truth(c, inp, out)
            _check(out, t, "out", dtype, False, tag)
            for key, x in (("dq", qd), ("dk", kd), ("dv", vd)):
                _check(x.grad, t, key, dtype, False, tag)
            if mode == "none":
                assert bd.grad is None
                continue
            want = base.double() + rep * t["r"]["dbias"]
            tr = dict(t, S=dict(t["S"], dbias=rep * t["S"]["dbias"]), AS=dict(t["AS"], dbias=rep * t["AS"]["dbias"]))
            _check(bd.grad, tr, "dbias", torch.float32, False, tag + f"backward {rep} ", extra=base.double().abs(), want=want)
            outside = torch.ones(c.H, c.Sb, c.Sb, dtype=torch.bool)
            outside[:, :c.Sq, :c.Skv] = False
            assert torch.equal(bd.grad.cpu()[outside], base[outside]), "the bias gradient changed outside [:, :Sq, :Skv]"


def test_wrapper_transposed_operands(lib):
    """Non-contiguous q, k, v and grad_output (transposed views) on the MFMA path and on the generic one."""
    ops = _ops()
    for c, paths in ((Case(3, 40, 77, 8), {FWD_MFMA: 1, BWD_MERGED: 1}), (Case(3, 40, 33, 2, 8, "fp32", 43), {GENERIC: 2})):
        inp, dtype, mfma = _inputs(c), DT[c.dt], GENERIC not in paths
        leaves = {n: inp[n].transpose(0, 1).contiguous().to(DEV).to(dtype).requires_grad_(True) for n in ("q", "k", "v")}
        qd, kd, vd = (leaves[n].transpose(0, 1) for n in ("q", "k", "v"))
        go = inp["go"].transpose(0, 1).contiguous().to(DEV).to(dtype).transpose(0, 1)
        assert not (qd.is_contiguous() or kd.is_contiguous() or vd.is_contiguous() or go.is_contiguous())
        bd = inp["bias"].float().to(DEV) if c.Sb else None
        before = ops.kernel_selections()
        out = ops.attention(qd, kd, vd, bd, c.H)
        out.backward(go)
        torch.cuda.synchronize()
        assert _launched(before) == paths
        t = _wrapper_truth(c, inp, out)
        _check(out, t, "out", dtype, mfma, "transposed views ")
        for key, n in (("dq", "q"), ("dk", "k"), ("dv", "v")):
            _check(leaves[n].grad.transpose(0, 1), t, key, dtype, mfma, "transposed views ")


def _bicubic_matrix(S0, S, ft=torch.float64):
    """R [S0 * S0][S * S]: F.interpolate(mode='bicubic', align_corners=False) as a matrix (its action on the unit tables)."""
    import torch.nn.functional as F
    eye = torch.eye(S0 * S0, dtype=ft).view(S0 * S0, 1, S0, S0)
    return F.interpolate(eye, size=(S, S), mode="bicubic", align_corners=False).view(S0 * S0, S * S)


def test_wrapper_bias_from_bicubic_resize(lib):
    """A bias that is the output of ops.bicubic_resize: a non-leaf; the table receives R^T dbias through it.  The attention reference
    takes the resized bias the kernel produced, so that only the gradient's path is measured.  Bound: K u |R|^T (|dbias| + A S), the
    scale of dbias carried through the magnitudes of the resize weights; K["dtable"] is calibrated like the others, with dbias and R
    evaluated in float32 (the kernel's resize backward adds with float atomics, in any order)."""
    ops = _ops()
    c, S0 = Case(3, 12, 12, 2, 8, "fp32", 12), 8
    inp = dict(_inputs(c))
    g = torch.Generator(device="cpu").manual_seed(4)
    table = (0.5 * torch.randn(c.H, S0, S0, generator=g)).to(DEV).requires_grad_(True)
    qd, kd, vd = (inp[n].to(DEV).float().requires_grad_(True) for n in ("q", "k", "v"))
    before = ops.kernel_selections()
    bias = ops.bicubic_resize(table, c.Sb)
    assert not bias.is_leaf
    out = ops.attention(qd, kd, vd, bias, c.H)
    out.backward(inp["go"].to(DEV).float())
    torch.cuda.synchronize()
    assert _launched(before) == {GENERIC: 2}
    inp["bias"] = bias.detach().cpu().double()
    t = _wrapper_truth(c, inp, out)
    _check(out, t, "out", torch.float32, False, "bicubic bias ")
    for key, x in (("dq", qd), ("dk", kd), ("dv", vd)):
        _check(x.grad, t, key, torch.float32, False, "bicubic bias ")
    R = _bicubic_matrix(S0, c.Sb)
    flat = lambda x: x.reshape(c.H, -1)                                                # noqa: E731
    want = (flat(t["r"]["dbias"]) @ R.t()).view(c.H, S0, S0)
    Sd = flat(t["r"]["dbias"]).abs() + flat(t["AS"]["dbias"])
    bound = ((K["dtable"] * U * Sd + flat(t["F"]["dbias"])) @ R.abs().t()).view(c.H, S0, S0)
    _match(table.grad, want, bound, (Sd @ R.abs().t()).view(c.H, S0, S0), "bicubic bias [generic float32] dtable", zeros=False)


def test_refusals(lib):
    """Host-checked and never launched: every output keeps its sentinel bits."""
    B, Sq, Skv, H, D = 2, 8, 8, 2, 4
    E = H * D
    x = torch.zeros(B, Sq, E, device=DEV)
    aux = torch.zeros(B, H, Sq, device=DEV)
    bias = torch.zeros(H, 8, 8, device=DEV)

    def go(B=B, Sq=Sq, Skv=Skv, D=D, Sb=0, bias=None, dbias=False, code=0, fwd=True, err="invalid argument"):
        outs = [Buf((2, 8, E), torch.float32) for _ in range(4)] + [Buf((2, H, 8), torch.float32), Buf((H, 8, 8), torch.float32)]
        o, dq, dk, dv, ls, db = outs
        before = _ops().kernel_selections()
        if fwd:
            with pytest.raises(RuntimeError, match=err):
                lib("hdmoe_attn_fwd", o.t, ls.t, x, x, x, bias, B, Sq, Skv, H, D, Sb, code)
        with pytest.raises(RuntimeError, match=err):
            lib("hdmoe_attn_bwd", dq.t, dk.t, dv.t, db.t if dbias else None, aux.clone(), x, x, x, x, x, aux, bias, B, Sq, Skv, H, D, Sb, code)
        torch.cuda.synchronize()
        assert _launched(before) == {}
        for b in outs:
            assert bool(b.base.isnan().all()) and b.margins_kept(), "a refused call wrote to an output"

    go(B=0)
    go(B=65536)
    go(Sq=0)
    go(Skv=0)
    go(Sq=8, Skv=4, Sb=7, bias=bias)         # Sb < Sq
    go(Sq=4, Skv=8, Sb=7, bias=bias)         # Sb < Skv
    go(dbias=True, fwd=False)                # dbias without bias
    go(D=3)
    go(D=64)
    go(code=2, err="unsupported dtype")
    go(code=7, err="unsupported dtype")
    before = _ops().kernel_selections()      # and the same calls inside the domain are taken
    lib("hdmoe_attn_fwd", x.clone(), aux.clone(), x, x, x, bias, B, Sq, Skv, H, D, 8, 0)
    lib("hdmoe_attn_bwd", x.clone(), x.clone(), x.clone(), bias.clone(), aux.clone(), x, x, x, x, x, aux, bias, B, Sq, Skv, H, D, 8, 0)
    torch.cuda.synchronize()
    assert _launched(before) == {GENERIC: 2}


# =====================================================================================================
# calibration (CPU only; `PYTHONPATH=. python tests/test_attention_kernels.py`)
# =====================================================================================================
def _bf(x):
    return x.float().bfloat16().double()


def _hi_lo(x, c32):
    """hi + lo bf16 pair of the fp32 product c x, as the kernels' scaled_frag carries it."""
    y = x.float() * c32
    hi = y.bfloat16().float()
    return (hi + (y - hi).bfloat16().float()).double()


def _expansion(x32, n):
    """n-term bf16 expansion of an fp32 tensor (shift_frag)."""
    tot, r = torch.zeros_like(x32, dtype=torch.float64), x32
    for _ in range(n):
        a = r.bfloat16().float()
        tot, r = tot + a.double(), r - a
    return tot


def _emulate_slice(inp, H, out_in=None, lse_in=None, first_tile=True, k_side=True):
    """The MFMA kernels' arithmetic in float64 with the roundings of their header and nothing else: c q (forward, dq kernel) or c k (merged,
    dk / dv kernel) as a hi + lo bf16 pair; forward: shift = the first tile's row maximum as a bf16 number (first_tile; the row maximum
    where that overflows fp32, as the repeated sweep has it, or always), p rounded to bf16 for both the output and the denominator;
    backward: -lse as a 2-term and -delta (an fp32 dot product) as a 3-term bf16 expansion, p and dS rounded to bf16 for the second product."""
    q, k, v, go = (_heads(inp[n], H) for n in ("q", "k", "v", "go"))
    c32 = torch.tensor(LOG2E, dtype=torch.float32) / math.sqrt(4.0)
    scale = 0.5
    s2 = _hi_lo(q, c32) @ k.transpose(-1, -2)
    rowmax = s2.amax(-1, keepdim=True)
    m = rowmax
    if first_tile and k.shape[2] <= 1024:
        m1 = _bf(s2[..., :32].amax(-1, keepdim=True))
        ok = ((s2 - m1).amax(-1, keepdim=True) < 127.0) & ((s2 - m1).amax(-1, keepdim=True) > -126.0)
        m = torch.where(ok, m1, rowmax)
    pt = _bf(torch.exp2(s2 - m))
    l = pt.sum(-1, keepdim=True)
    r = dict(out=_flat(pt @ v / l), lse=((m + torch.log2(l)) * LN2).squeeze(-1))
    s2 = (q @ _hi_lo(k, c32).transpose(-1, -2)) if k_side else s2
    nls = _expansion(-(lse_in.float() * torch.tensor(LOG2E, dtype=torch.float32)), 2)
    o = _heads(out_in, H)
    ndl = _expansion(-(go.float() * o.float()).sum(-1), 3)
    p = torch.exp2(s2 + nls[..., None])
    dS = p * (go @ v.transpose(-1, -2) + ndl[..., None])
    r.update(dv=_flat(_bf(p).transpose(-1, -2) @ go), dq=_flat(_bf(dS) @ k * scale), dk=_flat(_bf(dS).transpose(-1, -2) @ q * scale))
    return dict(r=r)


def _calibrate():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    tables = [("mfma", c) for c in MFMA_FWD + MERGED + PAIR] + [("generic", c) for c in MISALIGNED + [MANY_HEADS] + GENERIC_CASES]
    tables += [("generic", Case(3, 17, 145, 2, 8, "fp32", 148)), ("generic", Case(5, 33, 20, 2, 4, "bf16", 33)),
               ("generic", Case(3, 40, 33, 2, 8, "fp32", 43)), ("generic", Case(3, 40, 33, 2, 8, "bf16", 43)), ("mfma", Case(3, 40, 77, 8)),
               ("generic", Case(3, 12, 12, 2, 8, "fp32", 12)), ("generic", Case(2, 257, 129, 3, 8, "bf16", 260))]
    w32, wem, where32, whereem = dict.fromkeys(KEYS + ("dtable",), 0.0), dict.fromkeys(KEYS[:5], 0.0), {}, {}
    seen = set()
    for fam, c in tables:
        if c in seen:
            continue
        seen.add(c)
        inp, t = _inputs(c), _truth(c)
        if c.B * c.H * c.Sq * c.Skv <= 1 << 22:                  # the formulas ARE autograd's gradients (out_in = the exact out)
            leaves = {n: inp[n].clone().requires_grad_(True) for n in ("q", "k", "v")}
            bl = None if inp["bias"] is None else inp["bias"].clone().requires_grad_(True)
            qh, kh, vh = (_heads(leaves[n], c.H) for n in ("q", "k", "v"))
            s = qh @ kh.transpose(-1, -2) / math.sqrt(c.D)
            s = s if bl is None else s + bl[:, :c.Sq, :c.Skv]
            _flat(s.softmax(-1) @ vh).backward(inp["go"])
            ex = _formula(inp, c.H, scales=False)["r"]
            for key, x in (("dq", leaves["q"]), ("dk", leaves["k"]), ("dv", leaves["v"])) + ((("dbias", bl),) if bl is not None else ()):
                gr = x.grad if key != "dbias" else x.grad[:, :c.Sq, :c.Skv]
                assert float((gr - ex[key]).abs().max()) <= 1e-11 * (1.0 + float(ex[key].abs().max())), (key, _id(c))
        f32 = _formula(inp, c.H, ft=torch.float32, out_in=t["aux"]["out_in"], scales=False)["r"]
        for key in f32:
            unit = U * (t["r"][key].abs() + t["AS"][key])
            ratio = float((((f32[key] - t["r"][key]).abs() - t["F"][key]).clamp_min(0.0) / unit.clamp_min(1e-300)).max())
            if ratio > w32[key]:
                w32[key], where32[key] = ratio, _id(c)
        if c == Case(3, 12, 12, 2, 8, "fp32", 12):               # test_wrapper_bias_from_bicubic_resize: dtable = R^T dbias
            R, R32 = _bicubic_matrix(8, 12), _bicubic_matrix(8, 12, torch.float32)
            flat = lambda x: x.reshape(c.H, -1)                                        # noqa: E731
            unit = U * ((flat(t["r"]["dbias"]).abs() + flat(t["AS"]["dbias"])) @ R.abs().t())
            err = ((flat(f32["dbias"]).float() @ R32.t()).double() - flat(t["r"]["dbias"]) @ R.t()).abs()
            w32["dtable"], where32["dtable"] = float((err / unit).max()), _id(c)
        if fam == "mfma":
            for first_tile in (True, False):
                for k_side in (True, False):
                    em = _over_batch(_emulate_slice, inp, c.H, out_in=t["aux"]["out_in"], lse_in=t["r"]["lse"].float(), first_tile=first_tile,
                                     k_side=k_side)["r"]
                    for key in em:
                        unit = U * t["r"][key].abs() + 2.0 ** -8 * t["S"][key] + 2.0 ** -16 * t["AS"][key]
                        ratio = float((((em[key] - t["r"][key]).abs() - t["F"][key]).clamp_min(0.0) / unit.clamp_min(1e-300)).max())
                        if ratio > wem[key]:
                            wem[key], whereem[key] = ratio, _id(c)
        print(f"{fam:8s}{_id(c)}", flush=True)
    p2 = lambda x: 2.0 ** math.ceil(math.log2(4.0 * x))                               # noqa: E731
    for key in w32:
        line = f"  {key:9s}  {w32[key]:6.2f} ({where32.get(key)})  {4 * w32[key]:7.2f}  K = {p2(w32[key]):g}"
        if key in wem:
            line += f"   |   {wem[key]:6.3f} ({whereem.get(key)})  {4 * wem[key]:7.3f}  K_M = {p2(wem[key]):g}"
        print(line)


if __name__ == "__main__":
    _calibrate()
