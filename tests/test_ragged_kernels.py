"""The ragged-token kernels of the ViT expert bank against float64 on the CPU: csrc/ragged.hip (pack / unpack / select, gn_rag, ln_rag),
the ragged section of csrc/attention.hip (attn_rag_fwd / bwd / dbias) and the rel_pos_bias resize (bicubic_fwd / bwd).

Reference.  Inputs are drawn from a seed and rounded to the case's dtype; the same values are evaluated in float64 with plain torch, from
the definition and not from the padded layout: for every owned row r of expert g the first lens[g] tokens are sliced out and go through
F.group_norm (+ activation) or softmax attention with bias[g][:, :len, :len]; ln_rag is F.layer_norm over all Sp tokens of an owned row
(padding is normalised too: the kernel's contract); gradients come from autograd; padding tokens and unowned rows (at or past
seg[ngroups], or inside no expert's window) are exactly 0.  pack / unpack / select move bits and are compared bit for bit against the
index definition of the kernel comments (the pos_emb add of pack: one fp32 add, one rounding).  bicubic: F.interpolate(mode="bicubic",
align_corners=False) in float64 and its autograd gradient.  The padded, vectorised restatements (`_gn_formula`, `_ln_formula`,
`_attn_formula`, `_cubic_matrix`) give the scales of the bounds in float64 and the calibration of K in float32; the tests that are not
marked `gpu` prove them against the sliced torch results for random seg / lens.
The backward kernels take forward results as inputs.  gn_rag / ln_rag get the forward kernel's own fp32 mean / rstd (checked against the
float64 statistics first).  attn_rag_bwd gets `out` and `lse` of the float64 reference rounded to the case's dtype / fp32; for fp32 the
truth is autograd itself, for bf16 it is the float64 formula evaluated with that same rounded `out` (delta = sum dout * out is made of
it: one bf16 rounding of `out` moves dq by 2**-9 of its magnitude sum whatever the kernel does; the reference has to see the same
rounded values as the kernel).  `_attn_formula` equals autograd when `out` is exact (CPU test).

Bounds.  u = 2**-24; an fp32 output k must satisfy |k - r| <= K u (|r| + scale); a bf16 output adds 2**-8 |r|.  scale:
  out      max_j |v_j| of the row and head                     lse      max |score| of the row and head
  dq, dk   sum of p (|dp| + |delta|) |x| 1/sqrt(D) (x = k, q), |dp| = sum_d |dout_d v_d|, |delta| = sum_d |dout_d out_d|
  dv       sum_i p |dout_i|                                     dbias    sum over the expert's rows of p (|dp| + |delta|)
  gn_rag / ln_rag   the amp / mr scales of tests/test_norm_kernels.py: y (1 + max|z|) amp, dx amp rstd max|dz gamma|, dgamma / dbeta the
           magnitude sums of their terms, mean rms(x), rstd rstd E[x^2] / (var + eps); one element per group (var = 0): amp = 1
  bicubic  out |W| |table| |W|^T, dtable |W|^T |dout| |W| (W = the tap matrix);  dpos (pack_bwd)  sum |terms|
A parameter gradient that accumulates into a pre-filled tensor is compared with pre-fill + reference and gets |pre-fill| added to scale.
Zero and non-finite patterns: wherever the reference is exactly zero or non-finite the kernel must be, too.

K was set from the CPU and not from the kernels: `_calibrate` (run as `PYTHONPATH=. python tests/test_ragged_kernels.py`; never by a
test) evaluates the float32 restatements -- online-max softmax, two-pass centred variance, the cubic-tap polynomial -- over every case
table of this file; K = 4 x the worst ratio |fp32 CPU - fp64| / (u (|r| + scale)), rounded up to a power of two (the kernels sum in
another order and use __expf / __logf / rsqrtf).
  quantity                  worst fp32-CPU ratio      4 x      K       kernels' worst |err| / bound on the MI355X (fp32 outputs)
  gn_rag y                     2.99                   11.9     16      0.13
  gn_rag dx                    5.49                   22.0     32      0.08
  gn_rag dgamma / dbeta        4.75                   19.0     32      0.07
  gn_rag mean / rstd           3.07                   12.3     16      0.07
  ln_rag y                     1.45                    5.8      8      0.13
  ln_rag dx                    2.57                   10.3     16      0.12
  ln_rag dgamma / dbeta        2.65                   10.6     16      0.08
  ln_rag mean / rstd           1.39                    5.6      8      0.14
  attn out                    52.9                   211.8    256      0.19
  attn lse                     2.85                   11.4     16      0.10
  attn dq                    110.2                   440.7    512      0.12
  attn dk                    130.0                   520.0   1024      0.12
  attn dv                    223.0                   891.9   1024      0.25
  attn dbias                 240.9                   963.4   1024      0.06
  bicubic out               1477                    5909     8192      0.17
  bicubic dtable             680                    2719     4096      0.08
  pack_bwd dpos                1.76                    7.0      8      0.37
  The large attention ratios all come from the two cases with scores in the hundreds (elsewhere: out 2.8, dq 5.1, dk 3.9, dv 6.8,
  dbias 21): a score s carries an fp32 error of u |s|, exp turns it into a relative error of p, and the scales the bounds are stated in do
  not grow with |s|.  The bicubic ratios come from 64 -> 65 (16 -> 64, whose source coordinates are exact in fp32: 1.4): the source
  coordinate (dst + 0.5) S0 / S - 0.5 near 64 is good to 2**-18 in fp32, the taps are cubic in it, and |W| |table| |W|^T does not know.
  In the attention scales p enters as p + 2**-102: u 2**-102 = 2**-126 is fp32's smallest normal number, and a p below it may be flushed
  to zero (with scores in the hundreds most of a softmax row is).
  gn_rag's mean = 100 std case runs without activation and with ReLU only: through mp_silu' the error of z (amp u) reaches dz, which
  the dgamma / dbeta scales of the norm file do not carry (fp32-CPU ratio 35 there).

ReLU (gn_rag, act = 1).  Every ReLU case has <= 40k elements and draws seeds on the CPU until the float64 reference has no
pre-activation within 2 tau of zero, tau = the forward bound; the test asserts that before it launches.  No element is ever excluded.

Which arm each shape reaches.
* pack / unpack / select: one grid-stride loop, grid capped at 4096 x 256 threads.  L1 (the model's: an empty expert, two experts of one
  length, an unowned last row), L2 (lens 65 / 1 / 130), L3 (8 experts = HDMOE_MAX_GROUPS, a one-row expert); C = 1, 8, 32; with and without
  pos.  R = 129, lens (256, 64), C = 32: 1,056,768 elements > 4096 x 256, the loop takes a second trip.  select with 9 x 2 MiB rows:
  R row_bytes / 16 = 1,179,648 vectors > 1,048,576.
* gn_rag: one 256-thread block per row, strided over len x Cg per group.  (C, G) = (32, 4) the model's, (32, 32) Cg = 1, (32, 1) one
  group, (8, 2), (96, 32) 2 C = 192 floats of dynamic LDS, (256, 4).  len 4 x Cg 1: 4 of 256 threads busy; len 1 x Cg 1: one element per
  group; len 65 / 130: second trip of the strided loop at Cg >= 4 / 2; len = Sp and len = 4 in Sp = 130; mean = 100 std.
* ln_rag: CPL = 1 (C = 1, 8, 32), 2 (33, 48, 64), 4 (100, 128), 8 (129, 256) channels per lane, partial last lane groups at 1, 8, 33, 48,
  100, 129; 8 token slots per pass with Sp = 1, 5, 64, 130.
* attn_rag: one 64-lane block per (row, head), thread = query (fwd, dq) / key (dk, dv); D walks D_SWITCH = 1, 2, 4, 8, 16, 32; len 65 and
  130 cross the 64-lane loop edge; len 1: softmax of one key; sb = len + 3: the table's own stride; dbias: 8 row slices per element
  (gridDim.y), experts of 1, 7, 9 and 0 rows.
* bicubic: S0 -> S = 4 -> 9, 7 -> 10, 16 -> 64, 8 -> 8 (the table itself), 1 -> 5 (every tap clamps to the one entry), 64 -> 65; H = 1, 8.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import hdmoe_oracle as O

gpu = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS = 1e-5
NONE, RELU, SILU = 0, 1, 2
GUARD, MARK = 256, 777.0
NAN = float("nan")
DTYPES = [pytest.param(torch.float32, id="fp32"), pytest.param(torch.bfloat16, id="bf16")]
# K per quantity: see the table of the module docstring (set by _calibrate from the fp32 CPU restatements, not from the kernels)
K = dict(gn_y=16.0, gn_dx=32.0, gn_sum=32.0, gn_stat=16.0, ln_y=8.0, ln_dx=16.0, ln_sum=16.0, ln_stat=8.0,
         out=256.0, lse=16.0, dq=512.0, dk=1024.0, dv=1024.0, dbias=1024.0, bic_out=8192.0, bic_dt=4096.0, dpos=8.0)


# =====================================================================================================
# plumbing
# =====================================================================================================
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


def _dt(dtype):
    return 0 if dtype == torch.float32 else 1


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _rnd(t, dtype):
    return t.to(dtype).float()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _bound(r, scale, k, dtype=torch.float32):
    b = k * U * (r.abs().nan_to_num(0.0) + scale)
    return b + (2.0 ** -8 * r.abs().nan_to_num(0.0) if dtype == torch.bfloat16 else 0.0)


def _match(k, r, bound, msg, zeros=True, key=None):
    """k (device or CPU, any float) vs r (fp64 CPU): the same NaN and +-inf positions, exactly zero wherever r is exactly zero (zeros=False:
    r's zeros are cancellations), |k - r| <= bound elsewhere (bound: a float or a tensor broadcastable to r)."""
    k_dtype, k = k.dtype, k.detach().cpu().double()
    assert k.shape == r.shape, (msg, k.shape, r.shape)
    assert torch.equal(k.isnan(), r.isnan()), f"{msg}: NaN pattern {int(k.isnan().sum())} vs {int(r.isnan().sum())}"
    assert torch.equal(k.isinf(), r.isinf()) and torch.equal(k[k.isinf()], r[r.isinf()]), f"{msg}: inf pattern"
    if zeros:
        assert bool((k[r == 0] == 0).all()), f"{msg}: {int((k[r == 0] != 0).sum())} non-zeros where the reference is exactly zero"
    fin = torch.isfinite(r)
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(r)
    err = (k - r).abs()
    bad = fin & (err > b)
    worst = float((err[fin] / b[fin].clamp_min(1e-300)).max()) if fin.any() else 0.0
    print(f"{msg} [{str(k_dtype).replace('torch.', '')}] <{key}>: worst |err| / bound = {worst:.3f}")   # key: the docstring table's row
    assert not bad.any(), f"{msg}: {int(bad.sum())} entries over the bound, worst |err| {float(err[bad].max()):.3e} " \
                          f"at bound {float(b[bad][err[bad].argmax()]):.3e}"


class Lay:
    """A ragged layout: rows [seg[g], seg[g+1]) belong to expert g and hold lens[g] real tokens of Sp."""

    def __init__(self, lens, R, seg, Sp=None, name=""):
        self.lens, self.R, self.seg, self.G = list(lens), int(R), list(seg), len(lens)
        self.Sp = int(Sp) if Sp is not None else max(lens)
        self.name = name or f"lens={lens} seg={seg} R={R} Sp={self.Sp}"
        assert len(seg) == self.G + 1 and all(a <= b for a, b in zip(seg, seg[1:]))

    def owner(self):
        own = [-1] * self.R
        for g in range(self.G):
            for r in range(self.seg[g], min(self.seg[g + 1], self.R)):
                own[r] = g
        return own

    def rows(self):
        return [(r, g, self.lens[g]) for r, g in enumerate(self.owner()) if g >= 0]

    def own(self):
        gof = torch.tensor(self.owner(), dtype=torch.long)
        lenof = torch.tensor([self.lens[g] if g >= 0 else 0 for g in self.owner()], dtype=torch.long)
        return gof, lenof

    def alive(self):
        """(R, Sp) bool: the real tokens of owned rows."""
        return torch.arange(self.Sp)[None, :] < self.own()[1][:, None]

    def seg_dev(self):
        return torch.tensor(self.seg, dtype=torch.int32, device=DEV)

    def rag(self):
        assert self.Sp == max(self.lens)
        return _ops().RagLayout(self.seg_dev(), self.lens, self.R)


L1 = Lay([64, 16, 16, 4], 9, [0, 3, 3, 6, 8], name="L1")
L2 = Lay([65, 1, 130], 6, [0, 2, 3, 6], name="L2")
L3 = Lay([64, 1, 16, 4, 4, 16, 1, 64], 13, [0, 2, 3, 5, 5, 7, 9, 10, 12], name="L3")
L2_D32 = Lay([65, 1, 118], 6, [0, 2, 3, 6], name="L2 capped at the backward's D = 32 limit")
L_SMALL = Lay([65, 4], 2, [0, 1, 2], name="LS")                # ReLU at C = 96, 256: <= 40k elements
L_TINY = Lay([4, 2], 2, [0, 1, 2], name="tiny")
L_FULL = Lay([16], 2, [0, 2], name="len=Sp")
L_SHORT = Lay([4], 2, [0, 2], Sp=130, name="len=4 Sp=130")
L_DBIAS = Lay([16, 4, 8, 5], 18, [0, 1, 8, 17, 17], name="rows 1/7/9/0")
L_SP1 = Lay([1, 1], 3, [0, 1, 2], name="Sp=1")
L_SP5 = Lay([5, 2], 3, [0, 2, 3], name="Sp=5")


class _Outs:
    """Outputs inside guarded buffers: GUARD sentinel elements on both sides, the interior pre-filled (NaN: every element must be written)."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype, fill=NAN):
        n = int(math.prod(shape))
        buf = torch.full((GUARD + n + GUARD,), MARK, dtype=dtype, device=DEV)
        view = buf[GUARD:GUARD + n].view(*shape)
        if isinstance(fill, torch.Tensor):
            view.copy_(fill.to(DEV).to(dtype))
        else:
            view.fill_(fill)
        self.items.append((buf, n))
        return view

    def check(self, what):
        for i, (buf, n) in enumerate(self.items):
            assert bool((buf[:GUARD] == MARK).all()) and bool((buf[GUARD + n:] == MARK).all()), f"{what}: output {i} written out of bounds"


def _dead_zero(t, alive, what):
    """t (R, Sp, ...) on any device: exactly zero outside `alive` (R, Sp)."""
    t = t.detach().cpu()
    dead = ~alive
    assert bool((t[dead] == 0).all()), f"{what}: {int((t[dead] != 0).sum())} non-zero padding / unowned elements"


def _act(z, act):
    return F.relu(z) if act == RELU else (O.mp_silu(z) if act == SILU else z)


def _silu_grad_mag(z):
    sg = torch.sigmoid(z)
    return sg * (1.0 + z.abs() * (1.0 - sg)) / O.MP_SILU_DIV


def _per_expert(t, gof, G):
    """t (R, Sp, C) -> [sum over the rows of expert g and their tokens] per expert."""
    return [t[gof == g].sum((0, 1)) for g in range(G)]


# =====================================================================================================
# references: pack / unpack / select (index definitions, bit-exact), in the case's dtype on the CPU
# =====================================================================================================
def _pack_ref(srcs, pos, L, dtype):
    C = srcs[0].shape[-1]
    dst = torch.zeros(L.R, L.Sp, C, dtype=dtype)
    for r, g, n in L.rows():
        v = srcs[g][r].float()
        if pos is not None and pos[g] is not None:
            v = v + pos[g].reshape(n, C)                      # one fp32 add ...
        dst[r, :n] = v.to(dtype)                             # ... one rounding
    return dst


def _pack_bwd_ref(ddst, L, dtype):
    """every expert's full [R][len_e][C]: the gradient in its own rows, zero elsewhere;  dpos[g][s] = sum over g's rows (fp64)."""
    C = ddst.shape[-1]
    own = L.owner()
    dsrcs = [torch.zeros(L.R, n, C, dtype=dtype) for n in L.lens]
    dpos = [torch.zeros(n, C, dtype=torch.float64) for n in L.lens]
    mag = [torch.zeros(n, C, dtype=torch.float64) for n in L.lens]
    for r, g in enumerate(own):
        if g >= 0:
            n = L.lens[g]
            dsrcs[g][r] = ddst[r, :n]
            dpos[g] += ddst[r, :n].double()
            mag[g] += ddst[r, :n].double().abs()
    return dsrcs, dpos, mag


def _unpack_ref(src, L):
    return [src[:, :n].clone() for n in L.lens]


def _unpack_bwd_ref(ddsts, L, dtype):
    C = ddsts[0].shape[-1]
    acc = torch.zeros(L.R, L.Sp, C, dtype=torch.float32)
    for e, n in enumerate(L.lens):                           # the kernel adds the experts in this order, in fp32
        acc[:, :n] += ddsts[e].float()
    return acc.to(dtype)


def _select_ref(outs, L):
    y = torch.zeros_like(outs[0])
    for r, g in enumerate(L.owner()):
        if g >= 0:
            y[r] = outs[g][r]
    return y


def _select_bwd_ref(dy, L):
    douts = [torch.zeros_like(dy) for _ in range(L.G)]
    for r, g in enumerate(L.owner()):
        if g >= 0:
            douts[g][r] = dy[r]
    return douts


# =====================================================================================================
# references: gn_rag
# =====================================================================================================
def _gn_inputs(L, C, seed, dtype, mean=0.3, std=1.3):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    alive = L.alive()[..., None]
    x = _rnd(r(L.R, L.Sp, C) * std + mean, dtype) * alive
    dy = _rnd(r(L.R, L.Sp, C) + 0.25, dtype) * alive
    gms = [1 + 0.3 * r(C) for _ in range(L.G)]
    bts = [0.2 * r(C) for _ in range(L.G)]
    return x, gms, bts, dy


def _gn_ref(x, gms, bts, dy, L, G, act):
    """The truth: per owned row, F.group_norm over its first len tokens + activation, autograd gradients, fp64."""
    R, Sp, C = x.shape
    xr = x.double().clone().requires_grad_(True)
    gr = [t.double().clone().requires_grad_(True) for t in gms]
    br = [t.double().clone().requires_grad_(True) for t in bts]
    y, z = torch.zeros(R, Sp, C, dtype=torch.float64), torch.zeros(R, Sp, C, dtype=torch.float64)
    mean, rstd = torch.zeros(R, G, dtype=torch.float64), torch.zeros(R, G, dtype=torch.float64)
    loss = xr.sum() * 0.0
    for r, g, n in L.rows():
        xs = xr[r, :n]
        # (torch.group_norm is what F.group_norm calls after a size check that refuses one value per channel: len = 1)
        zz = torch.group_norm(xs.t()[None], G, gr[g], br[g], EPS)[0].t()
        yy = _act(zz, act)
        loss = loss + (yy * dy[r, :n].double()).sum()
        y[r, :n], z[r, :n] = yy.detach(), zz.detach()
        xg = xs.detach().reshape(n, G, C // G)
        mean[r] = xg.mean((0, 2))
        rstd[r] = (xg.var((0, 2), unbiased=False) + EPS).rsqrt()
    loss.backward()
    zero = torch.zeros(C, dtype=torch.float64)
    return dict(y=y, z=z, dx=xr.grad, dg=[t.grad if t.grad is not None else zero for t in gr],
                db=[t.grad if t.grad is not None else zero for t in br], mean=mean, rstd=rstd)


def _gn_formula(x, gms, bts, dy, L, G, act, ft=torch.float64):
    """gn_rag restated on the padded layout with the centred two-pass formulas of the kernel, in `ft`; fp64 also gives the scales."""
    R, Sp, C = x.shape
    Cg = C // G
    gof, lenof = L.own()
    gsel = gof.clamp_min(0)
    x, dy = x.to(ft), dy.to(ft)
    gm = torch.stack([t.to(ft) for t in gms])[gsel][:, None, :]
    bt = torch.stack([t.to(ft) for t in bts])[gsel][:, None, :]
    alive = L.alive()
    mk = alive[:, :, None, None]
    zero = torch.zeros((), dtype=ft)
    grp = lambda t: t.reshape(R, Sp, G, Cg)                                        # noqa: E731
    M = (lenof * Cg).clamp_min(1).to(ft).view(R, 1, 1, 1)
    xg = torch.where(mk, grp(x), zero)
    mean = xg.sum((1, 3), keepdim=True) / M
    d = torch.where(mk, xg - mean, zero)
    var = d.square().sum((1, 3), keepdim=True) / M
    rs = (var + EPS).rsqrt()
    xh = (d * rs).reshape(R, Sp, C)
    z = (xh * gm + bt).detach().requires_grad_(True)
    y = _act(z, act)
    (dz,) = torch.autograd.grad(y, z, torch.where(alive[..., None], dy, zero))
    y = torch.where(alive[..., None], y.detach(), zero)
    dz = torch.where(alive[..., None], dz, zero)
    z = z.detach()
    dzg = dz * gm
    s1, s2 = grp(dzg).sum((1, 3), keepdim=True), grp(dzg * xh).sum((1, 3), keepdim=True)
    dx = torch.where(mk, rs * (grp(dzg) - (s1 + grp(xh) * s2) / M), zero).reshape(R, Sp, C)
    res = dict(y=y, z=z, dx=dx, dg=_per_expert(dz * xh, gof, L.G), db=_per_expert(dz, gof, L.G), mean=mean.view(R, G), rstd=rs.view(R, G))
    if ft == torch.float64:
        ex = lambda t: t.reshape(R, 1, G, 1).expand(R, Sp, G, Cg).reshape(R, Sp, C)   # noqa: E731
        xa = xh.abs()
        mr = mean.abs() * rs
        mr = torch.where(M == 1, mr * U, mr)                 # one element per group: x - mean = 0 exactly
        mr = ex(mr)
        amp = 1.0 + mr * (1.0 + ex(grp(xa).amax((1, 3))))
        dza = torch.where(alive[..., None], dy.abs() * _silu_grad_mag(z), zero) if act == SILU else dz.abs()
        ex2 = torch.where(mk, grp(x), zero).square().sum((1, 3), keepdim=True) / M
        res["sc"] = dict(y=(1.0 + float(z.abs().max())) * amp, dx=amp * ex(rs) * ex(grp(dza * gm.abs()).amax((1, 3))),
                         dg=_per_expert(dza * (xa + mr * (1.0 + xa)), gof, L.G), db=_per_expert(dza, gof, L.G),
                         mean=ex2.sqrt().view(R, G), rstd=(rs * ex2 / (var + EPS)).view(R, G))
    return res


def _gn_relu_tau(ref, sc):
    return K["gn_y"] * U * (ref["z"].abs() + sc["y"])


def _gn_case_inputs(L, C, G, act, dtype, seed, **kw):
    """Inputs, truth and scales of one case; ReLU: the first seed (seed, seed + 1000, ...) whose fp64 pre-activations keep |z| > 2 tau."""
    for k in range(64):
        inp = _gn_inputs(L, C, seed + 1000 * k, dtype, **kw)
        ref = _gn_ref(*inp, L, G, act)
        sc = _gn_formula(*inp, L, G, act)["sc"]
        if act != RELU:
            return inp, ref, sc
        alive = L.alive()[..., None].expand_as(ref["z"])
        if bool((ref["z"].abs() > 2 * _gn_relu_tau(ref, sc))[alive].all()):
            assert inp[0].numel() <= 40000, "ReLU cases stay small"
            return inp, ref, sc
    raise AssertionError(f"gn_rag {L.name} C={C} G={G}: no seed keeps every ReLU pre-activation away from zero")


GN_CG = [(32, 4), (32, 32), (32, 1), (8, 2), (96, 32), (256, 4)]


def _gn_cases(act):
    """(tag, layout, C, G, kwargs): the (C, G) table over L1 and L2 (ReLU at C >= 96: the <= 40k-element LS) and the special cases."""
    cases = []
    for C, G in GN_CG:
        lays = [L1, L2] if not (act == RELU and C >= 96) else [L_SMALL]
        cases += [(f"gn_rag {L.name} C={C} G={G} act={act}", L, C, G, {}) for L in lays]
    cases.append((f"gn_rag len=Sp C=32 G=4 act={act}", L_FULL, 32, 4, {}))
    cases.append((f"gn_rag len=4 Sp=130 C=32 G=32 act={act}", L_SHORT, 32, 32, {}))
    # mean = 100 std: the forward bound (and so tau) is ~400 times wider; a ReLU case stays clear of 2 tau only with few elements.  Not with
    # mp_silu: there the error of z (amp u) passes through mp_silu' into dz, which the sum scales of the norm file do not carry.
    if act != SILU:
        cases.append((f"gn_rag mean=100std C=32 G=4 act={act}", L1 if act != RELU else L_TINY, 32, 4, dict(mean=100.0, std=1.0)))
    return cases


# =====================================================================================================
# references: ln_rag
# =====================================================================================================
LN_CS = [1, 8, 32, 33, 48, 64, 100, 128, 129, 256]
LN_LAYS = [L1, L2, L_SP1, L_SP5]


def _ln_inputs(L, C, seed, dtype, pad="zero", dy_pad=False):
    """pad: what the padding tokens of x hold -- zero, const (all equal: variance exactly 0) or junk (finite, different).  dy_pad: non-zero
    dy in the padding of owned rows."""
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    alive = L.alive()[..., None]
    x = _rnd(r(L.R, L.Sp, C) * 1.3 + 0.3, dtype)
    junk = _rnd(r(L.R, L.Sp, C) * 3.0 - 1.0, dtype)
    x = torch.where(alive, x, {"zero": torch.zeros_like(x), "const": torch.full_like(x, 0.5), "junk": junk}[pad])
    dy = _rnd(r(L.R, L.Sp, C) + 0.25, dtype)
    if not dy_pad:
        dy = dy * alive
    gms = [1 + 0.3 * r(C) for _ in range(L.G)]
    bts = [0.2 * r(C) for _ in range(L.G)]
    return x, gms, bts, dy


def _ln_ref(x, gms, bts, dy, L):
    """The truth: F.layer_norm over all Sp tokens of every owned row with its expert's affine; unowned rows 0; fp64 autograd."""
    R, Sp, C = x.shape
    xr = x.double().clone().requires_grad_(True)
    gr = [t.double().clone().requires_grad_(True) for t in gms]
    br = [t.double().clone().requires_grad_(True) for t in bts]
    y = torch.zeros(R, Sp, C, dtype=torch.float64)
    loss = xr.sum() * 0.0
    for r, g, _ in L.rows():
        yy = F.layer_norm(xr[r], (C,), gr[g], br[g], EPS)
        loss = loss + (yy * dy[r].double()).sum()
        y[r] = yy.detach()
    loss.backward()
    zero = torch.zeros(C, dtype=torch.float64)
    xd = x.double()
    return dict(y=y, dx=xr.grad, dg=[t.grad if t.grad is not None else zero for t in gr],
                db=[t.grad if t.grad is not None else zero for t in br], mean=xd.mean(-1),
                rstd=(xd.var(-1, unbiased=False) + EPS).rsqrt())


def _ln_formula(x, gms, bts, dy, L, ft=torch.float64):
    R, Sp, C = x.shape
    gof, _ = L.own()
    gsel = gof.clamp_min(0)
    owned = (gof >= 0).to(ft).view(R, 1, 1)
    x, dy = x.to(ft), dy.to(ft) * owned
    gm = torch.stack([t.to(ft) for t in gms])[gsel][:, None, :] * owned
    bt = torch.stack([t.to(ft) for t in bts])[gsel][:, None, :] * owned
    m = x.sum(-1, keepdim=True) / C
    d = x - m
    var = d.square().sum(-1, keepdim=True) / C
    rs = (var + EPS).rsqrt()
    xh = d * rs
    z = xh * gm + bt
    dzg = dy * gm
    a1, a2 = dzg.sum(-1, keepdim=True), (dzg * xh).sum(-1, keepdim=True)
    dx = rs * (dzg - (a1 + xh * a2) / C)
    res = dict(y=z, dx=dx, dg=_per_expert(dy * xh, gof, L.G), db=_per_expert(dy, gof, L.G), mean=m.squeeze(-1), rstd=rs.squeeze(-1))
    if ft == torch.float64:
        xa, dza = xh.abs(), dy.abs()
        mr = m.abs() * rs * (U if C == 1 else 1.0)
        amp = 1.0 + mr * (1.0 + xa.amax(-1, keepdim=True))
        ex2 = x.square().mean(-1, keepdim=True)
        res["sc"] = dict(y=(1.0 + float(z.abs().max())) * amp, dx=amp * rs * (dza * gm.abs()).amax(-1, keepdim=True),
                         dg=_per_expert(dza * (xa + mr * (1.0 + xa)), gof, L.G), db=_per_expert(dza, gof, L.G),
                         mean=ex2.sqrt().squeeze(-1), rstd=(rs * ex2 / (var + EPS)).squeeze(-1))
    return res


def _ln_cases():
    """(tag, layout, C, kwargs): every C over L1 / L2, Sp = 1 / 5 at one C per arm, the padding variants."""
    cases = [(f"ln_rag {L.name} C={C}", L, C, {}) for C in LN_CS for L in (L1, L2)]
    cases += [(f"ln_rag {L.name} C={C}", L, C, {}) for C in (8, 48, 100, 129) for L in (L_SP1, L_SP5)]
    cases += [(f"ln_rag L1 C={C} const padding, dy in the padding", L1, C, dict(pad="const", dy_pad=True)) for C in (32, 100)]
    cases += [(f"ln_rag L2 C={C} junk padding, dy in the padding", L2, C, dict(pad="junk", dy_pad=True)) for C in (33, 256)]
    return cases


# =====================================================================================================
# references: attn_rag
# =====================================================================================================
def _attn_inputs(L, H, D, seed, dtype, sb_extra=0, qk=1.0, big_bias=False):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    alive = L.alive()[..., None]
    E = H * D
    q, k = (_rnd(r(L.R, L.Sp, E) * qk, dtype) * alive for _ in range(2))
    v, dout = (_rnd(r(L.R, L.Sp, E) + 0.1, dtype) * alive for _ in range(2))
    biases = []
    for n in L.lens:
        b = r(H, n + sb_extra, n + sb_extra)
        biases.append(30.0 * torch.sign(b) if big_bias else 0.5 * b)
    return q, k, v, dout, biases


def _attn_ref(q, k, v, dout, biases, L, H):
    """The truth: per owned row and head, softmax(q k^T / sqrt(D) + bias[g][h, :len, :len]) v over the first len tokens; fp64 autograd."""
    R, Sp, E = q.shape
    D = E // H
    ql, kl, vl = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    bl = [b.double().clone().requires_grad_(True) for b in biases]
    out, lse = torch.zeros(R, Sp, E, dtype=torch.float64), torch.zeros(R, H, Sp, dtype=torch.float64)
    loss = ql.sum() * 0.0
    for r, g, n in L.rows():
        hv = lambda t: t[r, :n].reshape(n, H, D).transpose(0, 1)                   # noqa: E731
        s = hv(ql) @ hv(kl).transpose(1, 2) / math.sqrt(D) + bl[g][:, :n, :n]
        o = (torch.softmax(s, -1) @ hv(vl)).transpose(0, 1).reshape(n, E)
        loss = loss + (o * dout[r, :n].double()).sum()
        out[r, :n], lse[r, :, :n] = o.detach(), torch.logsumexp(s.detach(), -1)
    loss.backward()
    return dict(out=out, lse=lse, dq=ql.grad, dk=kl.grad, dv=vl.grad,
                dbias=[b.grad if b.grad is not None else torch.zeros_like(b) for b in bl])


def _attn_formula(q, k, v, dout, biases, L, H, ft=torch.float64, out_in=None, lse_in=None):
    """attn_rag restated with the kernels' formulas in `ft` (fp32: online-max softmax over the keys, as attn_rag_fwd_kernel runs it).
    out_in / lse_in: the forward results the backward is given (None: its own).  fp64 also gives the scales."""
    R, Sp, E = q.shape
    D = E // H
    scl = torch.tensor(float(D), dtype=ft).rsqrt()
    z = lambda *s: torch.zeros(*s, dtype=ft)                                       # noqa: E731
    res = dict(out=z(R, Sp, E), lse=z(R, H, Sp), dq=z(R, Sp, E), dk=z(R, Sp, E), dv=z(R, Sp, E), dbias=[z(*b.shape) for b in biases])
    sc = dict(out=z(R, Sp, E), lse=z(R, H, Sp), dq=z(R, Sp, E), dk=z(R, Sp, E), dv=z(R, Sp, E), dbias=[z(*b.shape) for b in biases])
    for r, g, n in L.rows():
        hv = lambda t: t[r, :n].to(ft).reshape(n, H, D).transpose(0, 1)            # noqa: E731
        back = lambda t: t.transpose(0, 1).reshape(n, E)                           # noqa: E731
        qs, ks, vs, do = hv(q) * scl, hv(k), hv(v), hv(dout)
        s = biases[g].to(ft)[:, :n, :n] + qs @ ks.transpose(1, 2)
        if ft == torch.float64:
            ls = torch.logsumexp(s, -1)
            o = torch.softmax(s, -1) @ vs
        else:
            m, l, o = torch.full((H, n), -math.inf, dtype=ft), z(H, n), z(H, n, D)
            for j in range(n):
                a = s[:, :, j]
                mn = torch.maximum(m, a)
                corr, p = torch.exp(m - mn), torch.exp(a - mn)
                l = l * corr + p
                o = o * corr[..., None] + p[..., None] * vs[:, j][:, None, :]
                m = mn
            o = o / l[..., None]
            ls = m + torch.log(l)
        res["out"][r, :n], res["lse"][r, :, :n] = back(o), ls
        oi = o if out_in is None else hv(out_in)
        li = ls if lse_in is None else lse_in[r, :, :n].to(ft)
        delta = (do * oi).sum(-1)
        p = torch.exp(s - li[..., None])
        dp = do @ vs.transpose(1, 2)
        ds = p * (dp - delta[..., None])
        res["dq"][r, :n], res["dk"][r, :n], res["dv"][r, :n] = back((ds @ ks) * scl), back(ds.transpose(1, 2) @ qs), back(p.transpose(1, 2) @ do)
        res["dbias"][g][:, :n, :n] += ds
        if ft == torch.float64:
            pw = p + 2.0 ** -102                             # u 2**-102 = 2**-126: a p below fp32's smallest normal number may be flushed to 0
            w = pw * (do.abs() @ vs.abs().transpose(1, 2) + (do.abs() * oi.abs()).sum(-1)[..., None])
            sc["out"][r, :n] = back(vs.abs().amax((1, 2), keepdim=True).expand(H, n, D))
            sc["lse"][r, :, :n] = s.abs().amax((1, 2), keepdim=True).expand(H, n, 1).squeeze(-1)
            sc["dq"][r, :n], sc["dk"][r, :n] = back((w @ ks.abs()) * scl), back(w.transpose(1, 2) @ qs.abs())
            sc["dv"][r, :n] = back(pw.transpose(1, 2) @ do.abs())
            sc["dbias"][g][:, :n, :n] += w
    if ft == torch.float64:
        res["sc"] = sc
    return res


def _attn_cases():
    """(tag, layout, H, D, kwargs)"""
    cases = [("attn_rag L1 H=8 D=4", L1, 8, 4, {}), ("attn_rag L3 H=3 D=4", L3, 3, 4, {}),
             ("attn_rag rows 1/7/9/0 H=2 D=4", L_DBIAS, 2, 4, {})]
    cases += [(f"attn_rag L2 H=2 D={D}", L2 if D < 32 else L2_D32, 2, D, {}) for D in (1, 2, 8, 16, 32)]
    cases += [("attn_rag L1 H=8 D=4 sb=len+3", L1, 8, 4, dict(sb_extra=3)), ("attn_rag L2 H=2 D=8 sb=len+3", L2, 2, 8, dict(sb_extra=3)),
              ("attn_rag L2 H=2 D=8 scores in the hundreds", L2, 2, 8, dict(qk=6.0, big_bias=True)),
              ("attn_rag L1 H=8 D=4 scores in the hundreds", L1, 8, 4, dict(qk=6.0, big_bias=True))]
    return cases


# =====================================================================================================
# references: bicubic
# =====================================================================================================
BICUBIC = [(4, 9), (7, 10), (16, 64), (8, 8), (1, 5), (64, 65)]


def _cubic_matrix(S0, S, ft=torch.float64):
    """W (S, S0): out = W table W^T per head -- the cubic-convolution taps of the kernel comments (A = -0.75, source coordinate
    (dst + 0.5) S0 / S - 0.5, taps clamped to the table), evaluated in `ft`."""
    A = -0.75
    scale = torch.tensor(float(S0), dtype=ft) / torch.tensor(float(S), dtype=ft)
    real = scale * (torch.arange(S, dtype=ft) + 0.5) - 0.5
    fl = torch.floor(real)
    t = real - fl
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    c = torch.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A, ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0,
                     ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A], 1)
    idx = (fl.long()[:, None] - 1 + torch.arange(4)[None, :]).clamp(0, S0 - 1)
    return torch.zeros(S, S0, dtype=ft).scatter_add_(1, idx, c), torch.zeros(S, S0, dtype=ft).scatter_add_(1, idx, c.abs())


def _bicubic_inputs(H, S0, S, seed):
    gen = _gen(seed)
    return torch.randn(H, S0, S0, generator=gen), torch.randn(H, S, S, generator=gen) + 0.25


def _bicubic_ref(table, g, S):
    t = table.double().clone().requires_grad_(True)
    out = F.interpolate(t[None], size=(S, S), mode="bicubic", align_corners=False)[0]
    out.backward(g.double())
    return dict(out=out.detach(), dt=t.grad)


def _bicubic_formula(table, g, S, ft=torch.float64):
    W, Wa = _cubic_matrix(table.shape[-1], S, ft)
    t, g = table.to(ft), g.to(ft)
    res = dict(out=W @ t @ W.t(), dt=W.t() @ g @ W)
    if ft == torch.float64:
        res["sc"] = dict(out=Wa @ t.abs() @ Wa.t(), dt=Wa.t() @ g.abs() @ Wa)
    return res


# =====================================================================================================
# CPU only: the restatements against the sliced torch truth; the library's domain query against its launchers
# =====================================================================================================
def _random_layout(gen, G, max_len):
    lens = [int(torch.randint(1, max_len + 1, (1,), generator=gen)) for _ in range(G)]
    cnt = [int(torch.randint(0, 4, (1,), generator=gen)) for _ in range(G)]
    seg = [0]
    for c in cnt:
        seg.append(seg[-1] + c)
    if seg[-1] == 0:
        seg[-1] = 1
    return Lay(lens, seg[-1] + int(torch.randint(0, 3, (1,), generator=gen)), seg)


def _tight(a, b, what, tol=1e-11):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), (what, float((a - b).abs().max()))


def test_reference_restatements_equal_the_sliced_torch_result():
    gen = _gen(1234)
    for trial in range(6):
        L = _random_layout(gen, 1 + trial % 5, 9)
        alive = L.alive()[..., None]
        for act in (NONE, RELU, SILU):
            inp = _gn_inputs(L, 12, 50 + trial, torch.float32)
            ref, f = _gn_ref(*inp, L, 3, act), _gn_formula(*inp, L, 3, act)
            for key in ("y", "dx"):
                _tight(f[key], ref[key], f"gn {key} {L.name}")
                assert bool((ref[key][~alive.expand_as(ref[key])] == 0).all()) and bool((f[key][~alive.expand_as(f[key])] == 0).all())
            own = L.own()[0] >= 0
            _tight(f["mean"][own], ref["mean"][own], "gn mean")
            _tight(f["rstd"][own], ref["rstd"][own], "gn rstd")
            for g in range(L.G):
                _tight(f["dg"][g], ref["dg"][g], "gn dgamma")
                _tight(f["db"][g], ref["db"][g], "gn dbeta")
        for kw in ({}, dict(pad="junk", dy_pad=True), dict(pad="const", dy_pad=True)):
            inp = _ln_inputs(L, 10, 70 + trial, torch.float32, **kw)
            ref, f = _ln_ref(*inp, L), _ln_formula(*inp, L)
            for key in ("y", "dx", "mean", "rstd"):
                _tight(f[key], ref[key], f"ln {key} {L.name}", 1e-9)
            for g in range(L.G):
                _tight(f["dg"][g], ref["dg"][g], "ln dgamma", 1e-9)
                _tight(f["db"][g], ref["db"][g], "ln dbeta", 1e-9)
        for sbx in (0, 2):
            inp = _attn_inputs(L, 2, 4, 90 + trial, torch.float32, sb_extra=sbx)
            ref, f = _attn_ref(*inp, L, 2), _attn_formula(*inp, L, 2)
            f32 = _attn_formula(*inp, L, 2, ft=torch.float32)
            for key in ("out", "lse", "dq", "dk", "dv"):
                _tight(f[key], ref[key], f"attn {key} {L.name}")
                _tight(f32[key].double(), ref[key], f"attn fp32 online {key}", 1e-4)
            for g in range(L.G):
                _tight(f["dbias"][g], ref["dbias"][g], "attn dbias")
                n = L.lens[g]
                outside = torch.ones_like(ref["dbias"][g], dtype=torch.bool)
                outside[:, :n, :n] = False
                assert bool((ref["dbias"][g][outside] == 0).all())
            dead = ~L.alive()
            assert bool((ref["out"][dead] == 0).all()) and bool((ref["dq"][dead] == 0).all()) and bool((ref["lse"].transpose(1, 2)[dead] == 0).all())
        # pack / unpack / select: round trips of the index definitions
        C = 3
        srcs = [torch.randn(L.R, n, C, generator=gen) for n in L.lens]
        packed = _pack_ref(srcs, None, L, torch.float32)
        parts = _unpack_ref(packed, L)
        for r, g, n in L.rows():
            assert torch.equal(parts[g][r], srcs[g][r]) and bool((packed[r, n:] == 0).all())
        dsrcs, dpos, _ = _pack_bwd_ref(packed, L, torch.float32)
        assert all(torch.equal(_unpack_bwd_ref(dsrcs, L, torch.float32), packed) for _ in (0,))
        for g in range(L.G):
            _tight(dpos[g], sum((srcs[g][r].double() for r, gg, _ in L.rows() if gg == g), torch.zeros(L.lens[g], C, dtype=torch.float64)), "dpos")
        outs = [torch.randn(L.R, 8, generator=gen) for _ in range(L.G)]
        y = _select_ref(outs, L)
        assert torch.equal(sum(_select_bwd_ref(y, L)), y)


@pytest.mark.parametrize("S0,S", BICUBIC)
def test_bicubic_reference(S0, S):
    """S = S0 returns the table; the tap matrix equals F.interpolate."""
    table, g = _bicubic_inputs(3, S0, S, 5)
    ref, f = _bicubic_ref(table, g, S), _bicubic_formula(table, g, S)
    _tight(f["out"], ref["out"], "bicubic out")
    _tight(f["dt"], ref["dt"], "bicubic dtable")
    if S == S0:
        assert torch.equal(ref["out"], table.double()) and torch.equal(f["out"], table.double())
        assert torch.equal(_bicubic_formula(table, g, S, torch.float32)["out"], table)


D_SWITCH = (1, 2, 4, 8, 16, 32)


def _raw_rag_attention(backward, n, D):
    """hdmoe_attn_rag_fwd / _bwd with one row of n tokens, one head: the status code (0 launched; without a GPU an accepted call comes
    back as -3 'launch failed', a refused one as -1 before any launch).  Real buffers where there is a GPU."""
    import ctypes
    from hdmoe_hip import _lib
    lib_ = _lib.lib()
    P = ctypes.c_void_p
    ints = lambda v: ctypes.cast((ctypes.c_int * len(v))(*v), P)                   # noqa: E731
    if torch.cuda.is_available():
        t = [torch.zeros(n * D, device=DEV) for _ in range(8)]
        tab, aux = torch.zeros(n * n, device=DEV), [torch.zeros(n, device=DEV) for _ in range(2)]
        seg = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
        ptr = lambda x: P(x.data_ptr())                                            # noqa: E731
        stream = P(torch.cuda.current_stream().cuda_stream)
    else:
        host = (ctypes.c_float * 16)()
        t, tab, aux, seg = [host] * 8, host, [host] * 2, host
        ptr = lambda x: P(ctypes.addressof(x))                                     # noqa: E731
        stream = None
    keep = (ctypes.c_void_p * 1)(ptr(tab).value)
    bias = ctypes.cast(keep, P)
    lens, sb = ints([n]), ints([n])
    if not backward:
        rc = lib_.hdmoe_attn_rag_fwd(ptr(t[0]), ptr(aux[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), bias, ptr(seg), lens, sb, 1, 1, n, 1, D, 0, stream)
    else:
        rc = lib_.hdmoe_attn_rag_bwd(ptr(t[0]), ptr(t[1]), ptr(t[2]), None, ptr(aux[1]), ptr(t[3]), ptr(t[4]), ptr(t[5]), ptr(t[6]), ptr(t[7]),
                                     ptr(aux[0]), bias, ptr(seg), lens, sb, 1, 1, n, 1, D, 0, stream)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
def test_attn_rag_max_len_is_the_launchers_limit(backward):
    """The query and the launcher agree on both sides of the edge, for every head dim of D_SWITCH; other head dims have no kernel."""
    from hdmoe_hip import ops
    for D in D_SWITCH:
        n = ops.attention_rag_max_len(D, bool(backward))
        assert n >= 1
        assert _raw_rag_attention(backward, n, D) != -1, (D, n)
        assert _raw_rag_attention(backward, n + 1, D) == -1, (D, n + 1)
        assert ops.attention_rag_max_len(D, True) < ops.attention_rag_max_len(D, False)
    for D in (0, 3, 5, 64):
        assert ops.attention_rag_max_len(D, bool(backward)) == 0 and _raw_rag_attention(backward, 4, D) == -1
    # the reproducer of the mismatch: D = 32, 119 tokens -- the forward takes it, the backward does not
    assert ops.attention_rag_max_len(32, False) >= 119 > ops.attention_rag_max_len(32, True)


def _edge_bank(device="cpu"):
    """Two ViT experts on an 11 x 11 image: patch 1 -> 121 tokens, patch 11 -> 1 token; C = 64, H = 2 -> D = 32."""
    import models.model_components as mc
    return torch.nn.ModuleList([mc.Vit_expert(num_heads=2, num_groups=4, in_channels=8, seq_ln=(11 // p) ** 2, emb_dim=64, num_blocks=1,
                                              patch_size=p, time_dim=6, text_dim=5) for p in (1, 11)]).to(device)


def test_vit_bank_compatible_asks_the_direction_it_will_run():
    """121 tokens at D = 32 lie inside the forward's limit and past the backward's: a bank only while no backward can follow."""
    import models.model_components as mc
    from hdmoe_hip import ops
    bank = list(_edge_bank())
    assert ops.attention_rag_max_len(32, True) < 121 <= ops.attention_rag_max_len(32, False)
    with torch.enable_grad():
        assert not mc.vit_bank_compatible(bank, 11, 11)
    with torch.no_grad():
        assert mc.vit_bank_compatible(bank, 11, 11)
    small = list(torch.nn.ModuleList([mc.Vit_expert(num_heads=2, num_groups=4, in_channels=8, seq_ln=(10 // p) ** 2, emb_dim=64, num_blocks=1,
                                                    patch_size=p, time_dim=6, text_dim=5) for p in (1, 10)]))
    with torch.enable_grad():
        assert mc.vit_bank_compatible(small, 10, 10)          # 100 tokens: inside both


# =====================================================================================================
# 1. pack / unpack / select
# =====================================================================================================
def _dev(ts, dtype=None):
    return [None if t is None else (t.to(DEV) if dtype is None else t.to(DEV).to(dtype)) for t in ts]


def _move_case(call, L, C, dtype, with_pos, seed, tag):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    R, Sp, G = L.R, L.Sp, L.G
    dt, seg = _dt(dtype), L.seg_dev()
    empty = [g for g in range(G) if L.seg[g] == L.seg[g + 1]]
    outs = _Outs()
    # pack
    srcs = [r(R, n, C).to(dtype) for n in L.lens]
    pos = [r(n, C) for n in L.lens] if with_pos else None
    dst = outs.new((R, Sp, C), dtype)
    call("hdmoe_rag_pack", dst, _dev(srcs), _dev(pos) if with_pos else None, seg, L.lens, G, R, Sp, C, dt)
    assert _same_bits(dst, _pack_ref(srcs, pos, L, dtype)), f"{tag}: pack"
    # pack_bwd: every expert's full tensor is written; dpos accumulates into the pre-fill; an empty expert's dpos keeps its bits
    ddst = r(R, Sp, C).to(dtype)
    dsrcs_ref, dpos_ref, dpos_mag = _pack_bwd_ref(ddst, L, dtype)
    dsrcs = [outs.new((R, n, C), dtype) for n in L.lens]
    base = [r(n, C) + 2.0 for n in L.lens]
    dpos = [outs.new((n, C), torch.float32, fill=b) for n, b in zip(L.lens, base)] if with_pos else None
    call("hdmoe_rag_pack_bwd", dsrcs, dpos, ddst.to(DEV), seg, L.lens, G, R, Sp, C, dt)
    for g in range(G):
        assert _same_bits(dsrcs[g], dsrcs_ref[g]), f"{tag}: pack_bwd expert {g}"
        if with_pos:
            want = base[g].double() + dpos_ref[g]
            _match(dpos[g], want, _bound(want, dpos_mag[g] + base[g].abs().double(), K["dpos"]), f"{tag}: dpos[{g}]", zeros=False, key="dpos")
            if g in empty:
                assert _same_bits(dpos[g], base[g]), f"{tag}: dpos of the empty expert {g} changed"
    # unpack: every expert's full tensor is written
    src = r(R, Sp, C).to(dtype)
    dsts = [outs.new((R, n, C), dtype) for n in L.lens]
    call("hdmoe_rag_unpack", dsts, src.to(DEV), seg, L.lens, G, R, Sp, C, dt)
    for g, want in enumerate(_unpack_ref(src, L)):
        assert _same_bits(dsts[g], want), f"{tag}: unpack expert {g}"
    # unpack_bwd
    ddsts = [r(R, n, C).to(dtype) for n in L.lens]
    dsrc = outs.new((R, Sp, C), dtype)
    call("hdmoe_rag_unpack_bwd", dsrc, _dev(ddsts), seg, L.lens, G, R, Sp, C, dt)
    assert _same_bits(dsrc, _unpack_bwd_ref(ddsts, L, dtype)), f"{tag}: unpack_bwd"
    # select / select_bwd over rows of 8 C elements (whole 16-byte vectors)
    n_el = 8 * C
    so = [r(R, n_el).to(dtype) for _ in range(G)]
    y = outs.new((R, n_el), dtype)
    nb = n_el * so[0].element_size()
    call("hdmoe_rag_select", y, _dev(so), seg, G, R, nb)
    assert _same_bits(y, _select_ref(so, L)), f"{tag}: select"
    dy = r(R, n_el).to(dtype)
    douts = [outs.new((R, n_el), dtype) for _ in range(G)]
    call("hdmoe_rag_select_bwd", douts, dy.to(DEV), seg, G, R, nb)
    for g, want in enumerate(_select_bwd_ref(dy, L)):
        assert _same_bits(douts[g], want), f"{tag}: select_bwd expert {g}"
    torch.cuda.synchronize()
    outs.check(tag)


@gpu
@pytest.mark.parametrize("with_pos", [False, True], ids=["nopos", "pos"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_unpack_select(lib, dtype, with_pos):
    for L in (L1, L2, L3):
        for C in (1, 8, 32):
            _move_case(lib, L, C, dtype, with_pos, 10 * C + L.G, f"{L.name} C={C}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_unpack_grid_stride(lib, dtype):
    """1,056,768 elements: past the 4096 x 256-thread grid cap, the loops take a second trip."""
    L = Lay([256, 64], 129, [0, 70, 128], name="R=129")
    assert L.R * L.Sp * 32 > 4096 * 256
    _move_case(lib, L, 32, dtype, True, 3, "grid-stride R=129 lens=(256, 64) C=32")


@gpu
def test_select_more_than_a_million_vectors(lib):
    L = Lay([1, 1], 9, [0, 4, 8], name="select-large")
    n_el = 524288                                            # 2 MiB fp32 rows: 9 x 2 MiB / 16 = 1,179,648 vectors, 18 MiB per tensor
    assert L.R * n_el * 4 // 16 > 1048576 and L.R * n_el * 4 < 32 << 20
    gen = _gen(4)
    so = [torch.randn(L.R, n_el, generator=gen) for _ in range(2)]
    outs = _Outs()
    y = outs.new((L.R, n_el), torch.float32)
    lib("hdmoe_rag_select", y, _dev(so), L.seg_dev(), 2, L.R, n_el * 4)
    assert _same_bits(y, _select_ref(so, L))
    douts = [outs.new((L.R, n_el), torch.float32) for _ in range(2)]
    lib("hdmoe_rag_select_bwd", douts, so[0].to(DEV), L.seg_dev(), 2, L.R, n_el * 4)
    for g, want in enumerate(_select_bwd_ref(so[0], L)):
        assert _same_bits(douts[g], want)
    outs.check("select-large")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_unpack_select_wrappers(lib, dtype):
    """ops.rag_pack / rag_unpack / rag_select through autograd; dpos accumulates into an existing .grad."""
    ops = _ops()
    for L in (L1, L2):
        gen = _gen(21 + L.G)
        r = lambda *s: torch.randn(*s, generator=gen)                              # noqa: E731
        C, rag = 8, L.rag()
        srcs = [r(L.R, n, C).to(dtype) for n in L.lens]
        pos = [r(1, n, C) for n in L.lens]
        base = [r(1, n, C) + 2.0 for n in L.lens]
        sd = [t.to(DEV).requires_grad_(True) for t in srcs]
        for accumulate in (False, True):
            pd = [t.to(DEV).requires_grad_(True) for t in pos]
            if accumulate:
                for p, b in zip(pd, base):
                    p.grad = b.to(DEV).clone()
            for t in sd:
                t.grad = None
            tok = ops.rag_pack(sd, pd, rag)
            assert _same_bits(tok, _pack_ref(srcs, pos, L, dtype)), f"{L.name}: ops.rag_pack"
            gt = r(L.R, L.Sp, C).to(dtype)
            tok.backward(gt.to(DEV))
            dsrcs_ref, dpos_ref, mag = _pack_bwd_ref(gt, L, dtype)
            for g in range(L.G):
                assert _same_bits(sd[g].grad, dsrcs_ref[g]), f"{L.name}: ops.rag_pack d(src {g})"
                b = base[g].double().view(-1, C) if accumulate else torch.zeros_like(dpos_ref[g])
                assert pd[g].grad is not None
                _match(pd[g].grad.view(-1, C), b + dpos_ref[g], _bound(b + dpos_ref[g], mag[g] + b.abs(), K["dpos"]),
                       f"{L.name}: ops.rag_pack dpos[{g}] accumulate={accumulate}", zeros=False, key="dpos")
        tk = r(L.R, L.Sp, C).to(dtype)
        td = tk.to(DEV).requires_grad_(True)
        parts = ops.rag_unpack(td, rag)
        gs = [r(L.R, n, C).to(dtype) for n in L.lens]
        for g, want in enumerate(_unpack_ref(tk, L)):
            assert _same_bits(parts[g], want), f"{L.name}: ops.rag_unpack {g}"
        torch.autograd.backward(list(parts), _dev(gs))
        assert _same_bits(td.grad, _unpack_bwd_ref(gs, L, dtype)), f"{L.name}: ops.rag_unpack backward"
        so = [r(L.R, 4, 8).to(dtype) for _ in range(L.G)]
        sod = [t.to(DEV).requires_grad_(True) for t in so]
        y = ops.rag_select(sod, rag)
        assert _same_bits(y, _select_ref(so, L)), f"{L.name}: ops.rag_select"
        gy = r(L.R, 4, 8).to(dtype)
        y.backward(gy.to(DEV))
        for g, want in enumerate(_select_bwd_ref(gy, L)):
            assert _same_bits(sod[g].grad, want), f"{L.name}: ops.rag_select d(out {g})"


# =====================================================================================================
# 2. gn_rag
# =====================================================================================================
def _gn_launch(call, inp, L, G, act, dtype, base_g, base_b, nan_pad=False):
    """Direct hdmoe_gn_rag_fwd + _bwd into guarded, NaN-pre-filled outputs; dgamma / dbeta pre-filled with base_*."""
    x, gms, bts, dy = inp
    R, Sp, C = x.shape
    if nan_pad:
        dead = ~L.alive()[..., None].expand_as(x)
        x, dy = x.clone(), dy.clone()
        x[dead], dy[dead] = NAN, NAN
    outs = _Outs()
    xd, dyd = x.to(DEV).to(dtype), dy.to(DEV).to(dtype)
    gd, bd = _dev(gms), _dev(bts)
    y, dx = outs.new((R, Sp, C), dtype), outs.new((R, Sp, C), dtype)
    mean, rstd = outs.new((R, G), torch.float32), outs.new((R, G), torch.float32)
    dg = [outs.new((C,), torch.float32, fill=b) for b in base_g]
    db = [outs.new((C,), torch.float32, fill=b) for b in base_b]
    seg, dt = L.seg_dev(), _dt(dtype)
    call("hdmoe_gn_rag_fwd", y, mean, rstd, xd, gd, bd, seg, L.lens, L.G, R, Sp, C, G, act, EPS, dt)
    call("hdmoe_gn_rag_bwd", dx, dg, db, dyd, xd, gd, bd, mean, rstd, seg, L.lens, L.G, R, Sp, C, G, act, dt)
    torch.cuda.synchronize()
    outs.check("gn_rag")
    return dict(y=y, dx=dx, mean=mean, rstd=rstd, dg=dg, db=db)


def _check_param_grads(got, ref, sc, base, L, k, tag, key):
    empty = [g for g in range(L.G) if L.seg[g] == L.seg[g + 1]]
    for g in range(L.G):
        want = base[g].double() + ref[g]
        _match(got[g], want, _bound(want, sc[g] + base[g].abs().double(), k), f"{tag}[{g}]", zeros=False, key=key)
        if g in empty:
            assert _same_bits(got[g], base[g]), f"{tag}[{g}]: the empty expert's gradient changed"


def _gn_check(call, tag, L, C, G, act, dtype, seed, **kw):
    inp, ref, sc = _gn_case_inputs(L, C, G, act, dtype, seed, **kw)
    alive = L.alive()
    if act == RELU:
        a3 = alive[..., None].expand_as(ref["z"])
        assert bool((ref["z"].abs() > 2 * _gn_relu_tau(ref, sc))[a3].all()), f"{tag}: a pre-activation within 2 tau of zero"
    gen = _gen(seed + 7)
    base_g = [torch.randn(C, generator=gen) + 2.0 for _ in range(L.G)]
    base_b = [torch.randn(C, generator=gen) - 2.0 for _ in range(L.G)]
    got = _gn_launch(call, inp, L, G, act, dtype, base_g, base_b)
    one = any(n * (C // G) == 1 for _, _, n in L.rows())     # one element per group somewhere: dx is a pure cancellation there
    _match(got["y"], ref["y"], _bound(ref["y"], sc["y"], K["gn_y"], dtype), f"{tag}: y", key="gn_y")
    _match(got["dx"], ref["dx"], _bound(ref["dx"], sc["dx"], K["gn_dx"], dtype), f"{tag}: dx", zeros=not one, key="gn_dx")
    _dead_zero(got["y"], alive, f"{tag}: y")
    _dead_zero(got["dx"], alive, f"{tag}: dx")
    own = L.own()[0] >= 0
    _match(got["mean"][own.to(DEV)], ref["mean"][own], _bound(ref["mean"][own], sc["mean"][own], K["gn_stat"]), f"{tag}: mean", zeros=False,
           key="gn_stat")
    _match(got["rstd"][own.to(DEV)], ref["rstd"][own], _bound(ref["rstd"][own], sc["rstd"][own], K["gn_stat"]), f"{tag}: rstd", key="gn_stat")
    assert bool(torch.isfinite(got["mean"]).all()) and bool(torch.isfinite(got["rstd"]).all())
    _check_param_grads(got["dg"], ref["dg"], sc["dg"], base_g, L, K["gn_sum"], f"{tag}: dgamma", "gn_sum")
    _check_param_grads(got["db"], ref["db"], sc["db"], base_b, L, K["gn_sum"], f"{tag}: dbeta", "gn_sum")
    # padding independence: NaN in the padding of x and dy changes no bit of a real token and the padding stays exactly zero
    nan = _gn_launch(call, inp, L, G, act, dtype, base_g, base_b, nan_pad=True)
    for key in ("y", "dx", "mean", "rstd"):
        assert _same_bits(nan[key], got[key]), f"{tag}: {key} depends on what the padding holds"


@gpu
@pytest.mark.parametrize("act", [NONE, RELU, SILU], ids=["none", "relu", "mp_silu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gn_rag(lib, dtype, act):
    for i, (tag, L, C, G, kw) in enumerate(_gn_cases(act)):
        _gn_check(lib, tag, L, C, G, act, dtype, 100 + i, **kw)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gn_rag_wrapper(lib, dtype):
    """ops.gn_rag through autograd: fresh parameter gradients, then accumulation into the existing .grad."""
    ops = _ops()
    for L, C, G, act in ((L1, 32, 4, SILU), (L2, 32, 32, NONE), (L1, 8, 2, RELU)):
        tag = f"ops.gn_rag {L.name} C={C} G={G} act={act}"
        inp, ref, sc = _gn_case_inputs(L, C, G, act, dtype, 300 + C + G)
        x, gms, bts, dy = inp
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        gd, bd = [t.to(DEV).requires_grad_(True) for t in gms], [t.to(DEV).requires_grad_(True) for t in bts]
        one = any(n * (C // G) == 1 for _, _, n in L.rows())
        for rep in (1, 2):                                   # the second backward finds .grad populated: the kernel adds into it
            xd.grad = None
            y = ops.gn_rag(xd, gd, bd, L.rag(), G, act, EPS)
            y.backward(dy.to(DEV).to(dtype))
            _match(y, ref["y"], _bound(ref["y"], sc["y"], K["gn_y"], dtype), f"{tag}: y", key="gn_y")
            _match(xd.grad, ref["dx"], _bound(ref["dx"], sc["dx"], K["gn_dx"], dtype), f"{tag}: dx", zeros=not one, key="gn_dx")
            for g in range(L.G):
                for got, r_, s_ in ((gd[g].grad, ref["dg"][g], sc["dg"][g]), (bd[g].grad, ref["db"][g], sc["db"][g])):
                    assert got is not None
                    _match(got, rep * r_, _bound(rep * r_, rep * s_, K["gn_sum"]), f"{tag}: param grad [{g}] after {rep}", zeros=False, key="gn_sum")


def _raises_einval(fn):
    with pytest.raises(RuntimeError, match="invalid argument"):
        fn()
    torch.cuda.synchronize()


@gpu
def test_gn_rag_rejections(lib):
    """G = 33, C % G != 0 and ngroups = 9 are refused on the host: HDMOE_EINVAL, nothing launched."""
    def go(C, G, ng):
        L = Lay([4] * ng, ng, list(range(ng + 1)))
        x = torch.zeros(L.R, 4, C, device=DEV)
        p = [torch.ones(C, device=DEV) for _ in range(ng)]
        st = torch.zeros(L.R * max(G, 1), device=DEV)
        fwd = lambda: lib("hdmoe_gn_rag_fwd", torch.empty_like(x), st, st.clone(), x, p, p, L.seg_dev(), L.lens, ng, L.R, 4, C, G, 0, EPS, 0)   # noqa: E731
        bwd = lambda: lib("hdmoe_gn_rag_bwd", torch.empty_like(x), p, p, x, x, p, p, st, st, L.seg_dev(), L.lens, ng, L.R, 4, C, G, 0, 0)        # noqa: E731
        return fwd, bwd
    for C, G, ng in ((66, 33, 2), (32, 3, 2), (32, 4, 9), (32, 0, 2)):
        for fn in go(C, G, ng):
            _raises_einval(fn)
    for fn in go(32, 4, 8):                                  # and the same call inside the domain is taken
        fn()
    torch.cuda.synchronize()


# =====================================================================================================
# 3. ln_rag
# =====================================================================================================
def _ln_launch(call, inp, L, dtype, base_g, base_b):
    x, gms, bts, dy = inp
    R, Sp, C = x.shape
    outs = _Outs()
    xd, dyd = x.to(DEV).to(dtype), dy.to(DEV).to(dtype)
    gd, bd = _dev(gms), _dev(bts)
    y, dx = outs.new((R, Sp, C), dtype), outs.new((R, Sp, C), dtype)
    mean, rstd = outs.new((R * Sp,), torch.float32), outs.new((R * Sp,), torch.float32)
    dg = [outs.new((C,), torch.float32, fill=b) for b in base_g]
    db = [outs.new((C,), torch.float32, fill=b) for b in base_b]
    seg, dt = L.seg_dev(), _dt(dtype)
    call("hdmoe_ln_rag_fwd", y, mean, rstd, xd, gd, bd, seg, L.G, R, Sp, C, EPS, dt)
    call("hdmoe_ln_rag_bwd", dx, dg, db, dyd, xd, gd, mean, rstd, seg, L.G, R, Sp, C, dt)
    torch.cuda.synchronize()
    outs.check("ln_rag")
    return dict(y=y, dx=dx, mean=mean.view(R, Sp), rstd=rstd.view(R, Sp), dg=dg, db=db)


def _ln_check(call, tag, L, C, dtype, seed, **kw):
    inp = _ln_inputs(L, C, seed, dtype, **kw)
    ref, sc = _ln_ref(*inp, L), _ln_formula(*inp, L)["sc"]
    gen = _gen(seed + 7)
    base_g = [torch.randn(C, generator=gen) + 2.0 for _ in range(L.G)]
    base_b = [torch.randn(C, generator=gen) - 2.0 for _ in range(L.G)]
    got = _ln_launch(call, inp, L, dtype, base_g, base_b)
    canc = C == 1 or kw.get("pad") in (None, "zero", "const")    # a token of equal channels: x - mean = 0, dx a pure cancellation
    _match(got["y"], ref["y"], _bound(ref["y"], sc["y"], K["ln_y"], dtype), f"{tag}: y", zeros=False, key="ln_y")
    _match(got["dx"], ref["dx"], _bound(ref["dx"], sc["dx"], K["ln_dx"], dtype), f"{tag}: dx", zeros=not canc, key="ln_dx")
    unowned = (L.own()[0] < 0)[:, None].expand(L.R, L.Sp)
    _dead_zero(got["y"], ~unowned, f"{tag}: y of unowned rows")
    _dead_zero(got["dx"], ~unowned, f"{tag}: dx of unowned rows")
    _match(got["mean"], ref["mean"], _bound(ref["mean"], sc["mean"], K["ln_stat"]), f"{tag}: mean", zeros=False, key="ln_stat")
    _match(got["rstd"], ref["rstd"], _bound(ref["rstd"], sc["rstd"], K["ln_stat"]), f"{tag}: rstd", key="ln_stat")
    _check_param_grads(got["dg"], ref["dg"], sc["dg"], base_g, L, K["ln_sum"], f"{tag}: dgamma", "ln_sum")
    _check_param_grads(got["db"], ref["db"], sc["db"], base_b, L, K["ln_sum"], f"{tag}: dbeta", "ln_sum")
    return inp, got


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_rag(lib, dtype):
    for i, (tag, L, C, kw) in enumerate(_ln_cases()):
        _ln_check(lib, tag, L, C, dtype, 400 + i, **kw)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_rag_real_tokens_do_not_see_the_padding(lib, dtype):
    """Finite junk instead of zeros in the padding tokens (ln_rag normalises them by contract): the real tokens keep every bit."""
    for L, C in ((L1, 32), (L2, 100), (L2, 256)):
        a = _ln_inputs(L, C, 77, dtype, pad="zero")
        b = _ln_inputs(L, C, 77, dtype, pad="junk")
        alive = L.alive()
        assert torch.equal(a[0][alive], b[0][alive]) and not torch.equal(a[0], b[0])
        zero = [torch.zeros(C) for _ in range(L.G)]
        ga, gb = _ln_launch(lib, a, L, dtype, zero, zero), _ln_launch(lib, b, L, dtype, zero, zero)
        for key in ("y", "dx", "mean", "rstd"):
            assert _same_bits(ga[key][alive.to(DEV)], gb[key][alive.to(DEV)]), f"ln_rag {L.name} C={C}: {key} of a real token saw the padding"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_rag_wrapper(lib, dtype):
    ops = _ops()
    for L, C in ((L1, 32), (L2, 48)):
        tag = f"ops.ln_rag {L.name} C={C}"
        inp = _ln_inputs(L, C, 500 + C, dtype)
        x, gms, bts, dy = inp
        ref, sc = _ln_ref(*inp, L), _ln_formula(*inp, L)["sc"]
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        gd, bd = [t.to(DEV).requires_grad_(True) for t in gms], [t.to(DEV).requires_grad_(True) for t in bts]
        for rep in (1, 2):
            xd.grad = None
            y = ops.ln_rag(xd, gd, bd, L.rag(), EPS)
            y.backward(dy.to(DEV).to(dtype))
            _match(y, ref["y"], _bound(ref["y"], sc["y"], K["ln_y"], dtype), f"{tag}: y", zeros=False, key="ln_y")
            _match(xd.grad, ref["dx"], _bound(ref["dx"], sc["dx"], K["ln_dx"], dtype), f"{tag}: dx", zeros=False, key="ln_dx")
            for g in range(L.G):
                for got, r_, s_ in ((gd[g].grad, ref["dg"][g], sc["dg"][g]), (bd[g].grad, ref["db"][g], sc["db"][g])):
                    assert got is not None
                    _match(got, rep * r_, _bound(rep * r_, rep * s_, K["ln_sum"]), f"{tag}: param grad [{g}] after {rep}", zeros=False, key="ln_sum")


@gpu
def test_ln_rag_rejections(lib):
    L = Lay([4, 4], 2, [0, 1, 2])
    x = torch.zeros(2, 4, 256, device=DEV)
    p = [torch.ones(257, device=DEV) for _ in range(2)]
    st = torch.zeros(8, device=DEV)
    for C in (0, 257):
        _raises_einval(lambda: lib("hdmoe_ln_rag_fwd", torch.empty_like(x), st, st.clone(), x, p, p, L.seg_dev(), 2, 2, 4, C, EPS, 0))
        _raises_einval(lambda: lib("hdmoe_ln_rag_bwd", torch.empty_like(x), p, p, x, x, p, st, st, L.seg_dev(), 2, 2, 4, C, 0))
    p9 = p * 5
    _raises_einval(lambda: lib("hdmoe_ln_rag_fwd", torch.empty_like(x), st, st.clone(), x, p9[:9], p9[:9], L.seg_dev(), 9, 2, 4, 256, EPS, 0))
    lib("hdmoe_ln_rag_fwd", torch.empty_like(x), st, st.clone(), x, p, p, L.seg_dev(), 2, 2, 4, 256, EPS, 0)
    torch.cuda.synchronize()


# =====================================================================================================
# 4. attn_rag
# =====================================================================================================
def _attn_launch(call, inp, L, H, dtype, out_in, lse_in, base, nan_pad=False):
    """Direct hdmoe_attn_rag_fwd, then hdmoe_attn_rag_bwd on (out_in, lse_in); guarded, NaN-pre-filled outputs, dbias pre-filled."""
    q, k, v, dout, biases = inp
    R, Sp, E = q.shape
    D = E // H
    if nan_pad:
        dead = ~L.alive()[..., None].expand_as(q)
        q, k, v, dout, out_in = (t.clone() for t in (q, k, v, dout, out_in))
        for t in (q, k, v, dout, out_in):
            t[dead] = NAN
    outs = _Outs()
    qd, kd, vd, dod, oid = (t.to(DEV).to(dtype) for t in (q, k, v, dout, out_in))
    lid = lse_in.float().to(DEV)
    bd = _dev(biases)
    sb = [int(b.shape[-1]) for b in biases]
    out, dq, dk, dv = (outs.new((R, Sp, E), dtype) for _ in range(4))
    lse = outs.new((R, H, Sp), torch.float32)
    delta = torch.zeros(R, H, Sp, device=DEV)
    dbias = [outs.new(tuple(b.shape), torch.float32, fill=b) for b in base]
    seg, dt = L.seg_dev(), _dt(dtype)
    call("hdmoe_attn_rag_fwd", out, lse, qd, kd, vd, bd, seg, L.lens, sb, L.G, R, Sp, H, D, dt)
    call("hdmoe_attn_rag_bwd", dq, dk, dv, dbias, delta, dod, oid, qd, kd, vd, lid, bd, seg, L.lens, sb, L.G, R, Sp, H, D, dt)
    torch.cuda.synchronize()
    outs.check("attn_rag")
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dbias=dbias)


def _attn_truth(inp, L, H, dtype):
    """(reference, scales, out / lse handed to the backward kernel).  fp32: autograd; bf16: the fp64 formula on the rounded `out`."""
    ref = _attn_ref(*inp, L, H)
    out_in, lse_in = _rnd(ref["out"], dtype), ref["lse"].float()
    f = _attn_formula(*inp, L, H, out_in=out_in, lse_in=lse_in)
    if dtype == torch.bfloat16:
        ref = dict(ref, dq=f["dq"], dk=f["dk"], dv=f["dv"], dbias=f["dbias"])
    return ref, f["sc"], out_in, lse_in


def _attn_check(call, tag, L, H, D, dtype, seed, **kw):
    inp = _attn_inputs(L, H, D, seed, dtype, **kw)
    ref, sc, out_in, lse_in = _attn_truth(inp, L, H, dtype)
    gen = _gen(seed + 7)
    base = [torch.randn(b.shape, generator=gen) + 2.0 for b in inp[4]]
    got = _attn_launch(call, inp, L, H, dtype, out_in, lse_in, base)
    alive = L.alive()
    # an expert of one token: p = 1 and dp - delta = dout.v - dout.out is a pure cancellation, so the reference's exact zeros in dq / dk
    # are not a pattern there; the padding's zeros are asserted on their own below
    one = any(n == 1 for _, _, n in L.rows())
    for key in ("out", "dq", "dk", "dv"):
        _match(got[key], ref[key], _bound(ref[key], sc[key], K[key], dtype), f"{tag}: {key}", zeros=not (one and key in ("dq", "dk")), key=key)
        _dead_zero(got[key], alive, f"{tag}: {key}")
        assert bool(torch.isfinite(got[key]).all())
    _match(got["lse"], ref["lse"], _bound(ref["lse"], sc["lse"], K["lse"]), f"{tag}: lse", key="lse")
    _dead_zero(got["lse"].transpose(1, 2), alive, f"{tag}: lse")
    empty = [g for g in range(L.G) if L.seg[g] == L.seg[g + 1]]
    for g in range(L.G):
        n = L.lens[g]
        want = base[g].double() + ref["dbias"][g]
        _match(got["dbias"][g], want, _bound(want, sc["dbias"][g] + base[g].abs().double(), K["dbias"]), f"{tag}: dbias[{g}]", zeros=False,
               key="dbias")
        outside = torch.ones(base[g].shape, dtype=torch.bool)
        outside[:, :n, :n] = False
        assert torch.equal(_bits(got["dbias"][g])[outside], _bits(base[g])[outside]), f"{tag}: dbias[{g}] written outside the len x len corner"
        if g in empty:
            assert _same_bits(got["dbias"][g], base[g]), f"{tag}: dbias of the empty expert {g} changed"
    # an expert of one token: a softmax of one key -- out is v, bit for bit
    for r, g, n in L.rows():
        if n == 1:
            assert _same_bits(got["out"][r, :1], inp[2][r, :1].to(dtype)), f"{tag}: row {r} (one token): out != v"
    # padding independence: NaN in the padding of q, k, v, dout (and out) changes no bit
    nan = _attn_launch(call, inp, L, H, dtype, out_in, lse_in, base, nan_pad=True)
    for key in ("out", "lse", "dq", "dk", "dv"):
        assert _same_bits(nan[key], got[key]), f"{tag}: {key} depends on what the padding holds"
    return got


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_rag(lib, dtype):
    for i, (tag, L, H, D, kw) in enumerate(_attn_cases()):
        _attn_check(lib, tag, L, H, D, dtype, 600 + i, **kw)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_rag_wrapper(lib, dtype):
    """ops.attention_rag with bias gradients fresh, accumulating into .grad, and with no bias requiring grad (dbias = None, no walker).
    bf16: `out` is saved rounded, so the truth of the gradients is the fp64 formula on that rounded `out` (module docstring)."""
    ops = _ops()
    L, H, D = L_DBIAS, 2, 4
    inp = _attn_inputs(L, H, D, 700, dtype)
    q, k, v, dout, biases = inp
    ref = _attn_ref(*inp, L, H)
    for mode in ("fresh", "accumulate", "none"):
        tag = f"ops.attention_rag biases {mode}"
        qd, kd, vd = (t.to(DEV).to(dtype).requires_grad_(True) for t in (q, k, v))
        bd = [b.to(DEV).requires_grad_(mode != "none") for b in biases]
        gen = _gen(9)
        base = [torch.randn(b.shape, generator=gen) + 2.0 if mode == "accumulate" else torch.zeros(b.shape) for b in biases]
        if mode == "accumulate":
            for b, b0 in zip(bd, base):
                b.grad = b0.to(DEV).clone()
        out = ops.attention_rag(qd, kd, vd, bd, L.rag(), H)
        out.backward(dout.to(DEV).to(dtype))
        f = _attn_formula(*inp, L, H, out_in=out.detach().cpu().float())
        tr = ref if dtype == torch.float32 else dict(ref, dq=f["dq"], dk=f["dk"], dv=f["dv"], dbias=f["dbias"])
        sc = f["sc"]
        _match(out, ref["out"], _bound(ref["out"], sc["out"], K["out"], dtype), f"{tag}: out", key="out")
        for key, t in (("dq", qd), ("dk", kd), ("dv", vd)):
            _match(t.grad, tr[key], _bound(tr[key], sc[key], K[key], dtype), f"{tag}: {key}", key=key)
        for g in range(L.G):
            if mode == "none":
                assert bd[g].grad is None
                continue
            want = base[g].double() + tr["dbias"][g]
            _match(bd[g].grad, want, _bound(want, sc["dbias"][g] + base[g].abs().double(), K["dbias"]), f"{tag}: dbias[{g}]", zeros=False, key="dbias")


@gpu
def test_attn_rag_rejections(lib):
    """Host-checked, never launched: a zero length, a length past Sp, a table smaller than the length, a null table, D = 3, a row past
    the LDS limit (forward: 241 tokens at D = 32; backward: 119, which the forward takes)."""
    def go(lens, Sp, sb, H, D, null_bias=False, bwd=True, fwd=True):
        G = len(lens)
        L = Lay(lens, G, list(range(G + 1)), Sp=Sp)
        E = H * D
        t = torch.zeros(G, Sp, E, device=DEV)
        aux = torch.zeros(G, H, Sp, device=DEV)
        bias = [None if null_bias else torch.zeros(H, max(s, 1), max(s, 1), device=DEV) for s in sb]
        fns = []
        if fwd:
            fns.append(lambda: lib("hdmoe_attn_rag_fwd", torch.empty_like(t), aux.clone(), t, t, t, bias, L.seg_dev(), lens, sb, G, G, Sp, H, D, 0))
        if bwd:
            fns.append(lambda: lib("hdmoe_attn_rag_bwd", torch.empty_like(t), torch.empty_like(t), torch.empty_like(t), None, aux.clone(), t, t, t,
                                   t, t, aux, bias, L.seg_dev(), lens, sb, G, G, Sp, H, D, 0))
        return fns
    bad = [go([4, 0], 4, [4, 4], 2, 4), go([4, 5], 4, [4, 5], 2, 4), go([4, 4], 4, [4, 3], 2, 4), go([4, 4], 4, [4, 4], 2, 4, null_bias=True),
           go([4, 4], 4, [4, 4], 2, 3), go([241], 241, [241], 1, 32), go([119], 119, [119], 1, 32, fwd=False)]
    for fns in bad:
        for fn in fns:
            _raises_einval(fn)
    for fn in go([4, 4], 4, [4, 4], 2, 4) + go([119], 119, [119], 1, 32, bwd=False):
        fn()
    torch.cuda.synchronize()


# =====================================================================================================
# batch independence: "a sample's output bits must not depend on its batch" (csrc/ragged.hip)
# =====================================================================================================
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_bits_do_not_depend_on_the_batch(lib, dtype):
    """One row alone (R = 1, one expert) and the same row at position 3 of an R = 7, 4-expert layout (expert 2): y, mean, rstd, out, lse, dx,
    dq, dk, dv come out bit-identical."""
    for n in (4, 16, 64, 65):
        big = Lay([16, 1, n, 8], 7, [0, 2, 2, 5, 7], Sp=max(n, 16))
        one = Lay([n], 1, [0, 1])
        at = 3
        zg = lambda C, G: [torch.zeros(C) for _ in range(G)]                        # noqa: E731
        # gn_rag (C = 32, G = 4, mp_silu) and ln_rag (C = 48)
        xb, gb, bb, dyb = _gn_inputs(big, 32, 800 + n, dtype)
        x1, dy1 = xb[at:at + 1, :n].clone(), dyb[at:at + 1, :n].clone()
        a = _gn_launch(lib, (xb, gb, bb, dyb), big, 4, SILU, dtype, zg(32, 4), zg(32, 4))
        b = _gn_launch(lib, (x1, [gb[2]], [bb[2]], dy1), one, 4, SILU, dtype, zg(32, 1), zg(32, 1))
        for key in ("y", "dx"):
            assert _same_bits(a[key][at, :n], b[key][0]), f"gn_rag len={n}: {key} depends on the batch"
        for key in ("mean", "rstd"):
            assert _same_bits(a[key][at], b[key][0]), f"gn_rag len={n}: {key} depends on the batch"
        xb, gb, bb, dyb = _ln_inputs(big, 48, 810 + n, dtype)
        x1, dy1 = xb[at:at + 1, :n].clone(), dyb[at:at + 1, :n].clone()
        a = _ln_launch(lib, (xb, gb, bb, dyb), big, dtype, zg(48, 4), zg(48, 4))
        b = _ln_launch(lib, (x1, [gb[2]], [bb[2]], dy1), one, dtype, zg(48, 1), zg(48, 1))
        for key in ("y", "dx", "mean", "rstd"):
            assert _same_bits(a[key][at, :n], b[key][0]), f"ln_rag len={n}: {key} depends on the batch"
        # attn_rag (H = 8, D = 4)
        H = 8
        q, k, v, do, bs = _attn_inputs(big, H, 4, 820 + n, dtype)
        ref = _attn_ref(q, k, v, do, bs, big, H)
        oi, li = _rnd(ref["out"], dtype), ref["lse"].float()
        a = _attn_launch(lib, (q, k, v, do, bs), big, H, dtype, oi, li, [torch.zeros_like(t) for t in bs])
        cut = lambda t: t[at:at + 1, :n].clone()                                   # noqa: E731
        b = _attn_launch(lib, (cut(q), cut(k), cut(v), cut(do), [bs[2]]), one, H, dtype, cut(oi), li[at:at + 1, :, :n].clone(),
                         [torch.zeros_like(bs[2])])
        for key in ("out", "dq", "dk", "dv"):
            assert _same_bits(a[key][at, :n], b[key][0]), f"attn_rag len={n}: {key} depends on the batch"
        assert _same_bits(a["lse"][at, :, :n], b["lse"][0]), f"attn_rag len={n}: lse depends on the batch"


# =====================================================================================================
# 5. bicubic
# =====================================================================================================
@gpu
@pytest.mark.parametrize("H", [1, 8])
def test_bicubic(lib, H):
    for S0, S in BICUBIC:
        tag = f"bicubic H={H} {S0}->{S}"
        table, g = _bicubic_inputs(H, S0, S, 40 + S)
        ref, sc = _bicubic_ref(table, g, S), _bicubic_formula(table, g, S)["sc"]
        outs = _Outs()
        out = outs.new((H, S, S), torch.float32)
        lib("hdmoe_bicubic_fwd", out, table.to(DEV), H, S0, S)
        base = torch.randn(H, S0, S0, generator=_gen(S)) + 2.0
        dt = outs.new((H, S0, S0), torch.float32, fill=base)
        lib("hdmoe_bicubic_bwd", dt, g.to(DEV), H, S0, S)
        torch.cuda.synchronize()
        outs.check(tag)
        _match(out, ref["out"], _bound(ref["out"], sc["out"], K["bic_out"]), f"{tag}: out", key="bic_out")
        want = base.double() + ref["dt"]
        _match(dt, want, _bound(want, sc["dt"] + base.abs().double(), K["bic_dt"]), f"{tag}: dtable", zeros=False, key="bic_dt")
        if S == S0:
            assert _same_bits(out, table), f"{tag}: S = S0 must return the table"


@gpu
def test_bicubic_wrapper(lib):
    H, S0, S = 8, 7, 10
    table, g = _bicubic_inputs(H, S0, S, 3)
    ref, sc = _bicubic_ref(table, g, S), _bicubic_formula(table, g, S)["sc"]
    td = table.to(DEV).requires_grad_(True)
    out = _ops().bicubic_resize(td, S)
    out.backward(g.to(DEV))
    _match(out, ref["out"], _bound(ref["out"], sc["out"], K["bic_out"]), "ops.bicubic_resize: out", key="bic_out")
    _match(td.grad, ref["dt"], _bound(ref["dt"], sc["dt"], K["bic_dt"]), "ops.bicubic_resize: dtable", zeros=False, key="bic_dt")


# =====================================================================================================
# the bank just past the backward's limit of the ragged attention
# =====================================================================================================
@gpu
def test_vit_bank_past_the_backward_limit_runs_per_expert_under_grad(lib):
    """D = 32, 121 tokens (11 x 11 image, patch 1), C = 64, H = 2: inside the forward's limit (240), past the backward's (118).  Under
    grad the per-expert path runs and its backward succeeds; under no_grad the bank path still runs; the two forwards agree."""
    import hdmoe_hip
    from hdmoe_hip import _lib, ops
    from models import _assembly as A
    hdmoe_hip.set_compute_dtype(torch.float32)
    assert ops.attention_rag_max_len(32, True) < 121 <= ops.attention_rag_max_len(32, False)
    torch.manual_seed(11)
    bank = _edge_bank(DEV)
    with torch.no_grad():
        for n, prm in bank.named_parameters():
            if "rel_pos_bias" in n or "pos_emb" in n:
                prm.normal_(0, 0.5)
    B = 3
    x = torch.randn(B, 8, 11, 11, device=DEV)
    te, text = torch.randn(B, 6, device=DEV), torch.randn(B, 5, device=DEV)
    w = torch.tensor([[1.0, 0.0], [0.0, 0.7], [0.4, 0.0]], device=DEV)

    def run(xx, ww):
        log = []
        _lib.CALL_LOG = log
        try:
            out = ops.from_nhwc(A._dispatch_nhwc(ops.to_nhwc(xx), bank, ww, te, text, kcap=1))
        finally:
            _lib.CALL_LOG = None
        return out, {name for name, _ in log}

    xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out, names = run(xx, ww)
    assert "hdmoe_attn_rag_fwd" not in names and "hdmoe_gn_rag_fwd" not in names, "under grad the bank path ran past the backward's limit"
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xx.grad).all()) and float(xx.grad.abs().max()) > 0
    grads = {n: p.grad for n, p in bank.named_parameters() if "rel_pos_bias" in n}
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    with torch.no_grad():
        out2, names2 = run(x, w)
    assert "hdmoe_attn_rag_fwd" in names2 and "hdmoe_gn_rag_fwd" in names2, "under no_grad the bank path must still run"
    scale = float(out.detach().abs().max())
    assert float((out2 - out.detach()).abs().max()) <= 1e-4 * scale, (float((out2 - out.detach()).abs().max()), scale)


# =====================================================================================================
# calibration of K (never run by a test):  PYTHONPATH=. python tests/test_ragged_kernels.py
# =====================================================================================================
def _calibrate():
    worst = {}

    def note(key, f32, ref, scale):
        ratio = float(((f32.double() - ref).abs() / (U * (ref.abs() + scale)).clamp_min(1e-300)).max()) if ref.numel() else 0.0
        worst[key] = max(worst.get(key, 0.0), ratio)

    for dtype in (torch.float32, torch.bfloat16):
        for act in (NONE, RELU, SILU):
            for i, (tag, L, C, G, kw) in enumerate(_gn_cases(act)):
                inp, ref, sc = _gn_case_inputs(L, C, G, act, dtype, 100 + i, **kw)
                f = _gn_formula(*inp, L, G, act, ft=torch.float32)
                own = L.own()[0] >= 0
                note("gn_y", f["y"], ref["y"], sc["y"]); note("gn_dx", f["dx"], ref["dx"], sc["dx"])
                note("gn_stat", f["mean"][own], ref["mean"][own], sc["mean"][own]); note("gn_stat", f["rstd"][own], ref["rstd"][own], sc["rstd"][own])
                for g in range(L.G):
                    note("gn_sum", f["dg"][g], ref["dg"][g], sc["dg"][g]); note("gn_sum", f["db"][g], ref["db"][g], sc["db"][g])
        for i, (tag, L, C, kw) in enumerate(_ln_cases()):
            inp = _ln_inputs(L, C, 400 + i, dtype, **kw)
            ref, sc, f = _ln_ref(*inp, L), _ln_formula(*inp, L)["sc"], _ln_formula(*inp, L, ft=torch.float32)
            note("ln_y", f["y"], ref["y"], sc["y"]); note("ln_dx", f["dx"], ref["dx"], sc["dx"])
            note("ln_stat", f["mean"], ref["mean"], sc["mean"]); note("ln_stat", f["rstd"], ref["rstd"], sc["rstd"])
            for g in range(L.G):
                note("ln_sum", f["dg"][g], ref["dg"][g], sc["dg"][g]); note("ln_sum", f["db"][g], ref["db"][g], sc["db"][g])
        for i, (tag, L, H, D, kw) in enumerate(_attn_cases()):
            inp = _attn_inputs(L, H, D, 600 + i, dtype, **kw)
            ref, sc, _, _ = _attn_truth(inp, L, H, torch.float32)
            f = _attn_formula(*inp, L, H, ft=torch.float32)
            for key in ("out", "lse", "dq", "dk", "dv"):
                note(key, f[key], ref[key], sc[key])
            for g in range(L.G):
                note("dbias", f["dbias"][g], ref["dbias"][g], sc["dbias"][g])
        for L in (L1, L2, L3, Lay([256, 64], 129, [0, 70, 128])):
            ddst = torch.randn(L.R, L.Sp, 8, generator=_gen(1)).to(dtype)
            _, dpos, mag = _pack_bwd_ref(ddst, L, dtype)
            own = L.owner()
            for g in range(L.G):
                acc = torch.zeros(L.lens[g], 8)
                for r in range(L.R):
                    if own[r] == g:
                        acc += ddst[r, :L.lens[g]].float()
                note("dpos", acc, dpos[g], mag[g])
    for H in (1, 8):
        for S0, S in BICUBIC:
            table, g = _bicubic_inputs(H, S0, S, 40 + S)
            ref, sc, f = _bicubic_ref(table, g, S), _bicubic_formula(table, g, S)["sc"], _bicubic_formula(table, g, S, torch.float32)
            note("bic_out", f["out"], ref["out"], sc["out"]); note("bic_dt", f["dt"], ref["dt"], sc["dt"])
    print(f"{'quantity':10s} {'worst fp32-CPU ratio':>22s} {'4 x':>8s} {'K':>6s} {'K in the file':>14s}")
    for key in K:
        w = worst.get(key, 0.0)
        k = 2.0 ** math.ceil(math.log2(max(4 * w, 1.0)))
        print(f"{key:10s} {w:22.2f} {4 * w:8.1f} {k:6.0f} {K[key]:14.0f}{'' if k == K[key] else '   <-- differs'}")


if __name__ == "__main__":
    _calibrate()
