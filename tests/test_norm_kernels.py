"""Every normalisation kernel of csrc/norm.hip against float64 on the CPU, on each path its host-side dispatch can take.

Reference.  Inputs are drawn from a seed and rounded to the case's dtype; the same values are evaluated in float64 (the truth:
F.layer_norm / F.group_norm / oracle.normalize / oracle.mp_silu with autograd gradients, and a short float64 restatement of the
formulas in the kernel comments for the GroupNorm(1, C) + ReLU router-trunk family) and in float32 (`_calibrate`, run as
`PYTHONPATH=. python tests/test_norm_kernels.py`; never by a test).  Kernels that take mean / rstd as inputs get the float64 statistics rounded
to fp32 and the reference uses those same fp32 values; hdmoe_gn1_finalize* are checked against the float64 sum of the same fp32
slot values.

Bounds.  u = 2**-24.  An fp32 output k must satisfy |k - r| <= K u (|r| + scale), scale = the largest magnitude the quantity passes
through before any cancellation.  With mr = |mean| rstd (what x - mean cancels from, in units of xhat; about 0.25 for the usual input
of mean 0.3, and 100 in the two cases whose mean is 100 standard deviations) and amp = 1 + mr (1 + max|xhat|) per row / group:
  y        (1 + max|z|) amp, z = the pre-activation (pixel-norm: 1 + max|xn|)
  dx       amp rstd max|dz gamma| per row / per (sample, group): the largest term of the sum dx is made of; where the activation is
           mp_silu, |dz| is |g| times the two terms of mp_silu' taken by magnitude (they cancel at z = -1.28).  Pixel-norm: the two terms
           of g / d - k2 x, with g = |sx dxn| + |dh mp_silu'|.  One element per group (var = 0): x - mean is exactly 0, amp = 1, and dx, a
           pure cancellation, gets this absolute part without a zero pattern
  sums     dgamma, dbeta, s1, s2, qsum: the sum of the magnitudes of their terms (for dgamma |dz| (|xhat| + mr (1 + |xhat|))).  Not the
           largest single term: the rounding of an n-term fp32 sum grows with n whatever the order (n = 524,300 rows here), and under the
           largest-term scale the CPU's own pairwise fp32 sums already reach ratios of 17 (2,100 rows) to 36 (3 x 1023 positions)
  mean     rms(x); rstd: rstd E[x^2] / (var + eps), what one rounding of E[x^2] does to it
bf16 outputs add 2**-8 |r| (one rounding to 8 significant bits); the fp32 statistics and dgamma / dbeta of a bf16 run do not.
Zero and non-finite patterns: wherever the reference is exactly zero or non-finite the kernel must be, too.

K is four times the worst ratio |fp32 CPU - fp64| / (u (|r| + scale)) that `_calibrate` measured over every case table of this file
(the kernels sum in another order and use fast rsqrt / exp), rounded up to a power of two.  The fp32 side is torch evaluating the same
references in float32: oracle.normalize / mp_silu with autograd for pixel-norm, the trunk restatement, and for LayerNorm / GroupNorm the
centred two-pass formulas of the kernel comments (`_gn_formula`).  F.layer_norm / F.group_norm in float32 are measured too but do not
set K for the gradients: torch's CPU backward uses the uncentred form (dx = a dy + b x + c), which no kernel here does.
  quantity      worst fp32-CPU ratio per family                                                              4 x worst   K
  y             layer_norm 1.41, group_norm 2.67, pixel_norm 2.55, trunk pool 0.53                             10.7       16
  dx            layer_norm 6.30 (at 524,300 x 3), group_norm 2.49, pixel_norm 3.28, trunk 2.80                 25.2       32
  sums          layer_norm 7.76 (C = 1: the sum is exactly 0 and the ratio is the fp64 reference's own
                rounding; 1.05 otherwise), group_norm 2.16, trunk s1 / s2 / dgamma / dbeta / qsum 2.31         31.0       32
  statistics    group_norm mean / rstd 3.77, trunk mean / one-pass rstd 0.68                                   15.1       16
  (F.layer_norm / F.group_norm in float32: y 1.59, dx 8.51 and 2.32; where the variance is exactly 0 -- C = 1, one element per group --
  their uncentred form does not cancel exactly: y is off by 254 of these units and the sums are not 0.  The kernels' centred form does.)
On the MI355X the kernels' own worst |error| / bound came out at 0.30 (y), 0.14 (dx), 0.24 (sums) and 0.05 (statistics) for fp32 outputs.

ReLU.  A pre-activation within fp32 rounding of zero may open in the kernel and not in the reference, which corrupts whole sums.  Every
ReLU case is small (<= ~40k elements) and draws seeds, on the CPU, until the float64 reference has no |z| <= 2 tau, tau = the forward
bound on z; the test asserts that before it runs the kernel.  No element is ever excluded.

Which kernel each shape reaches (W = 4 fp32 / 8 bf16 channels per 16-byte vector, LPR = pow2 >= C / W lanes per row):
* ops.layer_norm, ops.pixel_norm(_silu) -> {layernorm,pixelnorm}_{fwd,bwd}_vec_kernel<T, LPR> when C % W == 0, C / W <= 64 and every
  pointer is 16-byte aligned, else the one-thread-per-row kernels.
    fp32: C = 4 -> LPR 1, 8 -> 2, 12 -> 4 (3 of 4 lanes), 16 -> 4, 24 -> 8 (6), 36, 40 -> 16 (9, 10), 72 -> 32 (18), 132 -> 64 (33), 256 -> 64
          (full), 260 -> scalar (C / W = 65), 264, 512, 520 -> scalar (C / W > 64), 1, 3, 30 -> scalar (C % 4)
    bf16: C = 8 -> LPR 1, 16 -> 2, 24 -> 4 (3 of 4), 40 -> 8 (5), 72 -> 16 (9), 256 -> 32, 264 -> 64 (33), 512 -> 64 (full), 520 -> scalar
          (C / W = 65), 1, 3, 4, 12, 30, 36, 132, 260 -> scalar (C % 8)
    (16, 40 and 72 are there for the arms the other counts leave out: fp32 LPR 32, bf16 LPR 2, 8 and 16)
    rows = 16,400 (fp32 C = 256): 4100 blocks wanted, the forward's cap is 4096; rows = 2,100: 525 > the LayerNorm backward's 512;
    rows = 524,300 (C = 3): 2049 blocks > the scalar kernels' 2048.  A view one element into a buffer -> the scalar kernels.
* ops.group_norm -> groupnorm_{stats,bwd_stats,bwd_apply}_vec_kernel and groupnorm_apply_kernel<T, W> when C % W == 0, (C / G) % W == 0,
  cv = C / W divides 512 and the pointers are aligned, else the scalar kernels (thread -> group = t % G) and groupnorm_apply_kernel<T, 1>;
  forward row ranges (groupnorm_part_stats_vec_kernel + groupnorm_merge_kernel; the statistics body of both vector kernels is
  groupnorm_moments) when S >= 512, backward row ranges (atomics into s1 / s2) when N < 128 and S >= 256.  See GN_CASES.
* router trunks: direct calls, see the case tables of section 3.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import hdmoe_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS = 1e-5
K_Y, K_DX, K_SUM, K_STAT = 16.0, 32.0, 32.0, 16.0
NONE, RELU, SILU = 0, 1, 2
DTYPES = [pytest.param(torch.float32, id="fp32"), pytest.param(torch.bfloat16, id="bf16")]


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


def _bound(r, scale, K, dtype=torch.float32):
    b = K * U * (r.abs().nan_to_num(0.0) + scale)
    return b + (2.0 ** -8 * r.abs().nan_to_num(0.0) if dtype == torch.bfloat16 else 0.0)


def _match(k, r, bound, msg, zeros=True):
    """k (device, any float) vs r (fp64 CPU): the same NaN and +-inf positions, exactly zero wherever r is exactly zero (zeros=False: r's
    zeros are cancellations), |k - r| <= bound elsewhere (bound: a float or a tensor broadcastable to r)."""
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
    print(f"{msg} [{str(k_dtype).replace('torch.', '')}]: worst |err| / bound = {worst:.3f}")
    assert not bad.any(), f"{msg}: {int(bad.sum())} entries over the bound, worst |err| {float(err[bad].max()):.3e} " \
                          f"at bound {float(b[bad][err[bad].argmax()]):.3e}"


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _rnd(t, dtype):
    return t.to(dtype).float()


def _act(z, act):
    return F.relu(z) if act == RELU else (O.mp_silu(z) if act == SILU else z)


def _silu_grad_mag(z):
    """mp_silu'(z) = sigma (1 + z (1 - sigma)) / 0.596 with its two terms taken by magnitude (they cancel at z = -1.28)."""
    sg = torch.sigmoid(z)
    return sg * (1.0 + z.abs() * (1.0 - sg)) / O.MP_SILU_DIV


def _leaf(x, dtype, misaligned=False):
    """x on the device with requires_grad, and a function that returns its gradient.  misaligned: a contiguous view that starts one element
    into a larger leaf buffer, so its pointer is not 16-byte aligned."""
    if not misaligned:
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        return xd, lambda: xd.grad
    base = torch.zeros(x.numel() + 8, dtype=dtype, device=DEV)
    base[1:1 + x.numel()] = x.to(DEV).to(dtype).reshape(-1)
    base.requires_grad_(True)
    xd = base[1:1 + x.numel()].view(x.shape)
    assert xd.is_contiguous() and xd.data_ptr() % 16 != 0
    return xd, lambda: base.grad[1:1 + x.numel()].view(x.shape)


# =====================================================================================================
# references (ft = torch.float64: the truth; torch.float32: calibration only)
# =====================================================================================================
def _ln_ref(x, gm, bt, g, ft=torch.float64):
    xr, gr, br = (t.detach().to(ft).clone().requires_grad_(True) for t in (x, gm, bt))
    y = F.layer_norm(xr, (x.shape[-1],), gr, br, EPS)
    y.backward(g.to(ft))
    return dict(y=y.detach().double(), dx=xr.grad.double(), dg=gr.grad.double(), db=br.grad.double())


def _ln_scales(x, gm, bt, g):
    return _gn_scales(x.unsqueeze(1), gm, bt, g.unsqueeze(1), 1, NONE, squeeze=True)


def _pn_ref(x, dxn, dh, sx, ft=torch.float64):
    xr = x.detach().to(ft).clone().requires_grad_(True)
    xn = O.normalize(xr, dim=[1])
    h = O.mp_silu(xn)
    loss = 0.0
    if dxn is not None:
        loss = loss + (xn * dxn.to(ft)).sum() * sx
    if dh is not None:
        loss = loss + (h * dh.to(ft)).sum()
    loss.backward()
    return dict(xn=xn.detach().double(), h=h.detach().double(), dx=xr.grad.double())


def _pn_scales(x, dxn, dh, sx):
    x = x.double()
    C = x.shape[1]
    nrm = x.square().sum(1, keepdim=True).sqrt()
    inv = 1.0 / (1e-4 + nrm / math.sqrt(C))
    xn = (x * inv).requires_grad_(True)
    ga = torch.zeros_like(x)                                 # |sx dxn| + |dh mp_silu'(xn)|: the two parts of g may cancel
    if dxn is not None:
        ga = ga + abs(sx) * dxn.double().abs()
    if dh is not None:
        ga = ga + dh.double().abs() * _silu_grad_mag(xn.detach())
    k2 = torch.where(nrm > 0, (ga * x.abs()).sum(1, keepdim=True) * inv * inv / (math.sqrt(C) * nrm.clamp_min(1e-300)), torch.zeros_like(nrm))
    return dict(y=1.0 + float(xn.detach().abs().max()), dx=inv * ga.amax(1, keepdim=True) + k2 * x.abs().amax(1, keepdim=True))


def _gn_ref(x, gm, bt, g, G, act, ft=torch.float64):
    xr, gr, br = (t.detach().to(ft).clone().requires_grad_(True) for t in (x, gm, bt))
    z = F.group_norm(xr.transpose(1, 2), G, gr, br, EPS).transpose(1, 2)
    y = _act(z, act)
    y.backward(g.to(ft))
    return dict(y=y.detach().double(), z=z.detach().double(), dx=xr.grad.double(), dg=gr.grad.double(), db=br.grad.double())


def _gn_stats(x, G):
    """fp64 per-(sample, group) mean, biased variance and E[x^2] of x (N, S, C): each (N, G)."""
    N, S, C = x.shape
    xg = x.double().view(N, S, G, C // G)
    return xg.mean((1, 3)), xg.var((1, 3), unbiased=False), xg.square().mean((1, 3))


def _gn_formula(x, gm, bt, g, G, act, ft=torch.float64):
    """GroupNorm + activation and its gradients by the centred two-pass formulas the kernels implement (csrc/norm.hip), evaluated in `ft`:
    the scales of the bounds (fp64) and the calibration of K (fp32).  Also the per-(sample, group) statistics."""
    x, gm, bt, g = (t.detach().to(ft) for t in (x, gm, bt, g))
    N, S, C = x.shape
    M = S * (C // G)
    grp = lambda t: t.reshape(N, S, G, C // G)                                     # noqa: E731
    m = grp(x).mean((1, 3), keepdim=True)
    d = grp(x) - m
    var = d.square().mean((1, 3), keepdim=True)
    rs = (var + EPS).rsqrt()
    xh = (d * rs).reshape(N, S, C)
    z = (xh * gm + bt).requires_grad_(True)
    y = _act(z, act)
    (dz,) = torch.autograd.grad(y, z, g)
    dzg = dz * gm
    s1, s2 = grp(dzg).sum((1, 3), keepdim=True), grp(dzg * xh).sum((1, 3), keepdim=True)
    dx = (rs * (grp(dzg) - (s1 + grp(xh) * s2) / M)).reshape(N, S, C)
    return dict(y=y.detach(), z=z.detach(), dx=dx, dg=(dz * xh).sum((0, 1)), db=dz.sum((0, 1)), mean=m.view(N, G), rstd=rs.view(N, G),
                var=var.view(N, G), xh=xh, dz=dz, s1=s1, s2=s2, M=M)


def _gn_scales(x, gm, bt, g, G, act, squeeze=False):
    """The scales of the bounds (see the module docstring), from the fp64 formulas."""
    f = _gn_formula(x, gm, bt, g, G, act)
    N, S, C = x.shape
    ex = lambda t: t.reshape(N, 1, G, 1).expand(N, S, G, C // G).reshape(N, S, C)   # noqa: E731
    grp = lambda t: t.reshape(N, S, G, C // G)                                     # noqa: E731
    rs, xa = ex(f["rstd"]), f["xh"].abs()
    # x - mean cancels from |mean| rstd (in units of xhat): amp = 1 + that, times (1 + max|xhat|) for the sums xhat enters twice
    mr = ex(f["mean"].abs() * f["rstd"])
    if f["M"] == 1:                                          # one element per group: x - mean = 0 exactly; what is left is the fp64 reference's own rounding
        mr = mr * U
    amp = 1.0 + mr * (1.0 + ex(grp(xa).amax((1, 3))))
    dza = g.double().abs() * _silu_grad_mag(f["z"]) if act == SILU else f["dz"].abs()
    sc = dict(y=(1.0 + float(f["z"].abs().max())) * amp, dx=amp * rs * ex(grp(dza * gm.double().abs()).amax((1, 3))),
              dg=(dza * (xa + mr * (1.0 + xa))).sum((0, 1)), db=dza.sum((0, 1)))
    if squeeze:
        sc["y"], sc["dx"] = sc["y"].squeeze(1), sc["dx"].squeeze(1)
    return sc


def _gn1_ref(y, gm, bt, mean, rstd, dz=None, g=None, gscale=1.0, ft=torch.float64):
    """GroupNorm(1, C) + ReLU of y (N, S, C) with the given per-sample mean / rstd, as the kernel comments state it:
    xh = (y - mean) rstd, z = xh gamma + beta, dz' = dz [z > 0] (dz = g[n][c] gscale at every position in the pooled form),
    s1 = sum dz' gamma, s2 = sum dz' gamma xh, dgamma = sum dz' xh, dbeta = sum dz', dx = rstd (dz' gamma - (s1 + xh s2) / (S C)),
    pooled = mean_s relu(z), pcnt = #[z > 0], qsum = sum xh [z > 0]."""
    y, gm, bt, mean, rstd = (t.to(ft) for t in (y, gm, bt, mean, rstd))
    N, S, C = y.shape
    m, rs = mean.view(N, 1, 1), rstd.view(N, 1, 1)
    xh = (y - m) * rs
    z = xh * gm + bt
    opn = (z > 0).to(ft)
    r = dict(z=z, xh=xh, pooled=F.relu(z).mean(1), pcnt=opn.sum(1), qsum=(xh * opn).sum(1), sc_q=(xh * opn).abs().sum(1))
    if dz is not None or g is not None:
        d = dz.to(ft) if dz is not None else (g.to(ft) * gscale).view(N, 1, C).expand(N, S, C)
        dzz = d * opn
        s1, s2 = (dzz * gm).sum((1, 2)), (dzz * gm * xh).sum((1, 2))
        r.update(s1=s1, s2=s2, dg=(dzz * xh).sum((0, 1)), db=dzz.sum((0, 1)),
                 dx=rs * (dzz * gm - (s1.view(N, 1, 1) + xh * s2.view(N, 1, 1)) / (S * C)),
                 sc_dx=rs.abs() * (dzz * gm).abs().amax((1, 2), keepdim=True), sc_s1=(dzz * gm).abs().sum((1, 2)),
                 sc_s2=(dzz * gm * xh).abs().sum((1, 2)), sc_dg=(dzz * xh).abs().sum((0, 1)), sc_db=dzz.abs().sum((0, 1)))
    return {k: v.double() for k, v in r.items()}


def _relu_safe(make, zof, what):
    """make(seed) -> inputs; the first seed of 0, 1, .. whose fp64 pre-activations zof(inputs) keep |z| > 2 tau, tau = the forward bound."""
    for seed in range(64):
        inp = make(seed)
        z = zof(inp).double()
        tau = K_Y * U * (z.abs() + 1.0 + float(z.abs().max()))
        if bool((z.abs() > 2 * tau).all()):
            return inp
    raise AssertionError(f"{what}: no seed keeps every ReLU pre-activation away from zero")


def _assert_relu_safe(z, what):
    tau = K_Y * U * (z.abs() + 1.0 + float(z.abs().max()))
    assert bool((z.abs() > 2 * tau).all()), f"{what}: a reference pre-activation lies within the forward bound of zero"


# =====================================================================================================
# 1. row kernels: layer_norm, pixel_norm, pixel_norm_silu
# =====================================================================================================
ROW_CS = [1, 3, 4, 8, 12, 16, 24, 30, 36, 40, 72, 132, 256, 260, 264, 512, 520]
LONG_ROWS = [(16400, 256, torch.float32), (2100, 256, torch.float32), (524300, 3, torch.float32), (524300, 3, torch.bfloat16)]
LONG_IDS = ["16400x256-fp32", "2100x256-fp32", "524300x3-fp32", "524300x3-bf16"]


def _ln_inputs(rows, C, dtype, seed, mean=0.3, std=1.3):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    return _rnd(r(rows, C) * std + mean, dtype), 1 + 0.3 * r(C), 0.2 * r(C), _rnd(r(rows, C) + 0.25, dtype)


def _ln_hip(x, gm, bt, g, dtype, misaligned=False):
    xd, grad = _leaf(x, dtype, misaligned)
    gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
    y = _ops().layer_norm(xd, gd, bd, EPS)
    y.backward(g.to(DEV).to(dtype))
    return dict(y=y, dx=grad(), dg=gd.grad, db=bd.grad)


def _check_rows(tag, got, ref, sc, dtype, keys):
    for key, kind, K in keys:
        odt = dtype if kind in ("y", "dx") else torch.float32
        assert got[key].dtype == odt, (tag, key, got[key].dtype)
        _match(got[key], ref[key], _bound(ref[key], sc[kind if kind in sc else key], K, odt), f"{tag}: {key}")


LN_KEYS = [("y", "y", K_Y), ("dx", "dx", K_DX), ("dg", "dg", K_SUM), ("db", "db", K_SUM)]


def _ln_case(rows, C, dtype, seed, tag, **kw):
    x, gm, bt, g = _ln_inputs(rows, C, dtype, seed, **{k: v for k, v in kw.items() if k in ("mean", "std")})
    _check_rows(tag, _ln_hip(x, gm, bt, g, dtype, kw.get("misaligned", False)), _ln_ref(x, gm, bt, g),
                _ln_scales(x, gm, bt, g), dtype, LN_KEYS)


@pytest.mark.parametrize("rows", [1, 70])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_norm_channel_counts(dtype, rows):
    for C in ROW_CS:
        _ln_case(rows, C, dtype, 100 + C, f"layer_norm rows={rows} C={C}")


@pytest.mark.parametrize("rows,C,dtype", LONG_ROWS, ids=LONG_IDS)
def test_layer_norm_grid_stride(rows, C, dtype):
    _ln_case(rows, C, dtype, 7, f"layer_norm rows={rows} C={C}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_norm_mean_100_std(dtype):
    """A one-pass variance E[x^2] - mean^2 loses log2(1e4) = 13 bits here."""
    for C in (256, 30):
        _ln_case(70, C, dtype, 5, f"layer_norm mean=100 C={C}", mean=100.0, std=1.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_norm_misaligned_view(dtype):
    _ln_case(70, 32, dtype, 11, "layer_norm misaligned C=32", misaligned=True)
    _ln_case(70, 32, dtype, 11, "layer_norm aligned C=32")


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_norm_accumulates_into_existing_grads(dtype):
    for C in (32, 30):
        x, gm, bt, g = _ln_inputs(70, C, dtype, 13)
        ref, sc = _ln_ref(x, gm, bt, g), _ln_scales(x, gm, bt, g)
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
        for _ in range(2):                                   # the second backward finds .grad populated: the kernel adds into it
            _ops().layer_norm(xd, gd, bd, EPS).backward(g.to(DEV).to(dtype))
        _match(gd.grad, 2 * ref["dg"], _bound(2 * ref["dg"], 2 * sc["dg"], K_SUM), f"layer_norm C={C}: dgamma after two backwards")
        _match(bd.grad, 2 * ref["db"], _bound(2 * ref["db"], 2 * sc["db"], K_SUM), f"layer_norm C={C}: dbeta after two backwards")


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_kernels_row_independent(dtype):
    """Row 0 of a 70-row call and the 1-row call of that row: the same bits (LayerNorm and pixel-norm forward)."""
    ops = _ops()
    for C in ROW_CS:
        x, gm, bt, _ = _ln_inputs(70, C, dtype, 200 + C)
        xd, gd, bd = x.to(DEV).to(dtype), gm.to(DEV), bt.to(DEV)
        assert torch.equal(ops.layer_norm(xd, gd, bd, EPS)[0], ops.layer_norm(xd[:1].clone(), gd, bd, EPS)[0]), f"layer_norm C={C}"
        a, b = ops.pixel_norm_silu(xd), ops.pixel_norm_silu(xd[:1].clone())
        assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]), f"pixel_norm_silu C={C}"
        assert torch.equal(ops.pixel_norm(xd)[0], ops.pixel_norm(xd[:1].clone())[0]), f"pixel_norm C={C}"


def _pn_inputs(rows, C, dtype, seed):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    return _rnd(r(rows, C) * 1.3 + 0.3, dtype), _rnd(r(rows, C) + 0.25, dtype), _rnd(0.7 * r(rows, C) - 0.2, dtype)


def _pn_hip(x, dxn, dh, sx, dtype, silu, misaligned=False):
    xd, grad = _leaf(x, dtype, misaligned)
    if silu:
        xn, h = _ops().pixel_norm_silu(xd, sx)
        torch.autograd.backward([xn, h], [dxn.to(DEV).to(dtype), dh.to(DEV).to(dtype)])
    else:
        assert sx == 1.0
        xn, h = _ops().pixel_norm(xd), None
        xn.backward(dxn.to(DEV).to(dtype))
    return dict(xn=xn, h=h, dx=grad())


def _pn_case(x, dxn, dh, sx, dtype, silu, tag, misaligned=False):
    if not silu:
        dh = None
    got = _pn_hip(x, dxn, dh, sx, dtype, silu, misaligned)
    ref, sc = _pn_ref(x, dxn, dh, sx), _pn_scales(x, dxn, dh, sx)
    _check_rows(tag, got, ref, sc, dtype, [("xn", "y", K_Y), ("dx", "dx", K_DX)] + ([("h", "y", K_Y)] if silu else []))


@pytest.mark.parametrize("silu,sx", [(False, 1.0), (True, 1.0), (True, 0.3)], ids=["plain", "silu", "silu-gx0.3"])
@pytest.mark.parametrize("rows", [1, 70])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pixel_norm_channel_counts(dtype, rows, silu, sx):
    for C in ROW_CS:
        _pn_case(*_pn_inputs(rows, C, dtype, 300 + C), sx, dtype, silu, f"pixel_norm rows={rows} C={C} silu={silu} gx={sx}")


@pytest.mark.parametrize("rows,C,dtype", LONG_ROWS, ids=LONG_IDS)
def test_pixel_norm_grid_stride(rows, C, dtype):
    _pn_case(*_pn_inputs(rows, C, dtype, 9), 0.3, dtype, True, f"pixel_norm rows={rows} C={C}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_pixel_norm_misaligned_view(dtype):
    _pn_case(*_pn_inputs(70, 32, dtype, 17), 0.3, dtype, True, "pixel_norm misaligned C=32", misaligned=True)
    _pn_case(*_pn_inputs(70, 32, dtype, 17), 0.3, dtype, True, "pixel_norm aligned C=32")


def _pn_edge_rows(C, dtype, seed):
    """8 rows: row 2 all zero (k2 = 0 branch), row 4 of magnitude 1e-6 (norm << eps = 1e-4), row 5 of magnitude 1e4."""
    x, dxn, dh = _pn_inputs(8, C, torch.float32, seed)
    x[2] = 0.0
    x[4] *= 1e-6
    x[5] *= 1e4
    return _rnd(x, dtype), _rnd(dxn, dtype), _rnd(dh, dtype)


@pytest.mark.parametrize("C", [3, 8, 24, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pixel_norm_zero_tiny_and_huge_rows(dtype, C):
    x, dxn, dh = _pn_edge_rows(C, dtype, 400 + C)
    _pn_case(x, dxn, dh, 0.3, dtype, True, f"pixel_norm edge rows C={C} silu")
    _pn_case(x, dxn, dh, 1.0, dtype, False, f"pixel_norm edge rows C={C}")


@pytest.mark.parametrize("C", [3, 24, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pixel_norm_bwd_with_one_gradient_missing(lib, dtype, C):
    """hdmoe_pixelnorm_bwd with dxn = None (only the silu output has a consumer) and with dh = None."""
    x, dxn, dh = _pn_edge_rows(C, dtype, 500 + C)
    xd = x.to(DEV).to(dtype)
    for a, b, sx, what in ((None, dh, 1.0, "dxn=None"), (dxn, None, 0.3, "dh=None")):
        dx = torch.full_like(xd, float("nan"))
        lib("hdmoe_pixelnorm_bwd", dx, None if a is None else a.to(DEV).to(dtype), None if b is None else b.to(DEV).to(dtype), xd,
            x.shape[0], C, sx, _dt(dtype))
        ref, sc = _pn_ref(x, a, b, sx), _pn_scales(x, a, b, sx)
        _match(dx, ref["dx"], _bound(ref["dx"], sc["dx"], K_DX, dtype), f"pixelnorm_bwd C={C} {what}")
    with pytest.raises(RuntimeError):
        lib("hdmoe_pixelnorm_bwd", dx, None, None, xd, x.shape[0], C, 1.0, _dt(dtype))


# =====================================================================================================
# 2. GroupNorm
# =====================================================================================================
# (N, S, C, G, act): what it reaches
GN_CASES = [
    (2, 5, 8, 1, RELU),          # fewer vectors than threads (vector kernels, cv = 2 / 1)
    (2, 7, 24, 8, NONE),         # C / G = 3: scalar kernels in both dtypes, thread -> group = t % 8
    (3, 33, 32, 8, SILU),        # C / G = 4: fp32 vector, bf16 scalar
    (1, 9, 256, 64, NONE),       # G = 64, fp32 vector (cv = 64), bf16 scalar
    (1, 9, 512, 64, SILU),       # G = 64, both vector (cv = 128 / 64)
    (1, 3, 2048, 1, RELU),       # fp32 cv = 512: vec_group_reduce's tree loop runs zero times
    (2, 2, 4096, 32, SILU),      # bf16 cv = 512; fp32 cv = 1024 > 512: scalar kernels with 32 KB of dynamic LDS
    (4, 1, 8, 8, NONE),          # one element per group: var = 0, y = beta
    (2, 513, 16, 2, SILU),       # forward parts 2 (257 + 256 rows), backward parts 4 (129 x 3 + 126)
    (3, 1023, 32, 4, NONE),      # forward parts 3 (341 x 3: full-length last range), backward parts 7 (147 x 6 + 141)
    (1, 1025, 8, 1, RELU),       # forward parts 4 (257 x 3 + 254), backward parts 8 (129 x 7 + 122)
    (130, 256, 8, 1, SILU),      # N >= 128: backward unsplit
]
GN_IDS = ["-".join(map(str, c)) for c in GN_CASES]


def _gn_make(N, S, C, G, act, dtype, seed, mean=0.3, std=1.3):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    return _rnd(r(N, S, C) * std + mean, dtype), 1 + 0.3 * r(C), 0.2 * r(C), _rnd(r(N, S, C) + 0.25, dtype)


def _gn_inputs(N, S, C, G, act, dtype, base_seed, **kw):
    if act != RELU:
        return _gn_make(N, S, C, G, act, dtype, base_seed, **kw)
    assert N * S * C <= 41000
    return _relu_safe(lambda s: _gn_make(N, S, C, G, act, dtype, base_seed + 1000 * s, **kw),
                      lambda t: _gn_ref(t[0], t[1], t[2], t[3], G, act)["z"], f"group_norm {(N, S, C, G)}")


def _gn_hip(x, gm, bt, g, G, act, dtype, misaligned=False):
    xd, grad = _leaf(x, dtype, misaligned)
    gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
    y = _ops().group_norm(xd, gd, bd, G, act, EPS)
    y.backward(g.to(DEV).to(dtype))
    return dict(y=y, dx=grad(), dg=gd.grad, db=bd.grad)


def _gn_check(tag, got, x, gm, bt, g, G, act, dtype, var0=False):
    ref, sc = _gn_ref(x, gm, bt, g, G, act), _gn_scales(x, gm, bt, g, G, act)
    if act == RELU:
        _assert_relu_safe(ref["z"], tag)
    odt = got["y"].dtype
    assert odt == dtype and got["dx"].dtype == dtype and got["dg"].dtype == torch.float32 and got["db"].dtype == torch.float32
    _match(got["y"], ref["y"], _bound(ref["y"], sc["y"], K_Y, dtype), f"{tag}: y")
    if var0:                                                 # dx = rstd (dz gamma - dz gamma): a cancellation, the absolute part alone
        _match(got["dx"], ref["dx"], K_DX * U * sc["dx"], f"{tag}: dx", zeros=False)
    else:
        _match(got["dx"], ref["dx"], _bound(ref["dx"], sc["dx"], K_DX, dtype), f"{tag}: dx")
    _match(got["dg"], ref["dg"], _bound(ref["dg"], sc["dg"], K_SUM), f"{tag}: dgamma", zeros=not var0)
    _match(got["db"], ref["db"], _bound(ref["db"], sc["db"], K_SUM), f"{tag}: dbeta")
    return ref


@pytest.mark.parametrize("N,S,C,G,act", GN_CASES, ids=GN_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_paths(dtype, N, S, C, G, act):
    x, gm, bt, g = _gn_inputs(N, S, C, G, act, dtype, 31 + S + C)
    tag = f"group_norm {(N, S, C, G, act)}"
    got = _gn_hip(x, gm, bt, g, G, act, dtype)
    _gn_check(tag, got, x, gm, bt, g, G, act, dtype, var0=(S * (C // G) == 1))
    if S * (C // G) == 1:                                    # x - mean = 0 exactly in the kernels' centred form
        assert torch.equal(got["y"].cpu().float(), bt.to(dtype).float().expand(N, S, C)), f"{tag}: y = beta"


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_mean_100_std(dtype):
    N, S, C, G = 2, 300, 16, 2
    x, gm, bt, g = _gn_inputs(N, S, C, G, NONE, dtype, 41, mean=100.0, std=1.0)
    _gn_check("group_norm mean=100", _gn_hip(x, gm, bt, g, G, NONE, dtype), x, gm, bt, g, G, NONE, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_misaligned_view(dtype):
    N, S, C, G = 2, 33, 32, 4
    x, gm, bt, g = _gn_inputs(N, S, C, G, SILU, dtype, 43)
    _gn_check("group_norm misaligned", _gn_hip(x, gm, bt, g, G, SILU, dtype, misaligned=True), x, gm, bt, g, G, SILU, dtype)
    _gn_check("group_norm aligned", _gn_hip(x, gm, bt, g, G, SILU, dtype), x, gm, bt, g, G, SILU, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_accumulates_into_existing_grads(dtype):
    for (N, S, C, G) in ((2, 33, 32, 4), (2, 7, 24, 8), (2, 513, 16, 2)):
        x, gm, bt, g = _gn_inputs(N, S, C, G, SILU, dtype, 47)
        ref, sc = _gn_ref(x, gm, bt, g, G, SILU), _gn_scales(x, gm, bt, g, G, SILU)
        xd = x.to(DEV).to(dtype).requires_grad_(True)
        gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
        for _ in range(2):
            _ops().group_norm(xd, gd, bd, G, SILU, EPS).backward(g.to(DEV).to(dtype))
        _match(gd.grad, 2 * ref["dg"], _bound(2 * ref["dg"], 2 * sc["dg"], K_SUM), f"group_norm {(N, S, C, G)}: dgamma after two backwards")
        _match(bd.grad, 2 * ref["db"], _bound(2 * ref["db"], 2 * sc["db"], K_SUM), f"group_norm {(N, S, C, G)}: dbeta after two backwards")


def _stat_bounds(x, G):
    m, var, ex2 = _gn_stats(x, G)
    rs = (var + EPS).rsqrt()
    return m, rs, _bound(m, ex2.sqrt(), K_STAT), _bound(rs, rs * ex2 / (var + EPS), K_STAT)


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_split_with_mostly_empty_row_ranges(lib, dtype):
    """hdmoe_groupnorm_fwd_split / _bwd_split with parts = 64 at S = 130: ranges of 3 rows, the 44th holds one row, 20 are empty."""
    N, S, C, G, parts = 2, 130, 16, 2, 64
    x, gm, bt, g = _gn_make(N, S, C, G, SILU, dtype, 53)
    ref, sc = _gn_ref(x, gm, bt, g, G, SILU), _gn_scales(x, gm, bt, g, G, SILU)
    xd, gd, bd, gg = x.to(DEV).to(dtype), gm.to(DEV), bt.to(DEV), g.to(DEV).to(dtype)
    y = torch.full_like(xd, float("nan"))
    mean, rstd = torch.full((N * G,), float("nan"), device=DEV), torch.full((N * G,), float("nan"), device=DEV)
    ws = torch.full((2 * N * parts * G,), float("nan"), device=DEV)
    lib("hdmoe_groupnorm_fwd_split", y, mean, rstd, ws, parts, xd, gd, bd, N, S, C, G, SILU, EPS, _dt(dtype))
    m, rs, bm, brs = _stat_bounds(x, G)
    _match(mean.view(N, G), m, bm, "fwd_split: mean")
    _match(rstd.view(N, G), rs, brs, "fwd_split: rstd")
    _match(y, ref["y"], _bound(ref["y"], sc["y"], K_Y, dtype), "fwd_split: y")
    dx = torch.full_like(xd, float("nan"))
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ws2 = torch.zeros(2 * N * G, device=DEV)                  # the row-range blocks add into it
    lib("hdmoe_groupnorm_bwd_split", dx, dg, db, ws2, parts, gg, xd, gd, bd, mean, rstd, N, S, C, G, SILU, _dt(dtype))
    _match(dx, ref["dx"], _bound(ref["dx"], sc["dx"], K_DX, dtype), "bwd_split: dx")
    _match(dg, ref["dg"], _bound(ref["dg"], sc["dg"], K_SUM), "bwd_split: dgamma")
    _match(db, ref["db"], _bound(ref["db"], sc["db"], K_SUM), "bwd_split: dbeta")


@pytest.mark.parametrize("N,S,C", [(3, 40, 16), (65, 17, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_bwd_bcast(lib, dtype, N, S, C):
    """hdmoe_groupnorm_bwd_bcast: the gradient of mean_s relu(GN(1, C)(x)) under the cotangent g[n][c], nothing of size N S C read but x."""
    def make(seed):
        gen = _gen(61 + 1000 * seed)
        r = lambda *s: torch.randn(*s, generator=gen)                              # noqa: E731
        return _rnd(r(N, S, C) * 1.3 + 0.3, dtype), 1 + 0.3 * r(C), 0.2 * r(C), r(N, C) + 0.25
    x, gm, bt, g = _relu_safe(make, lambda t: _gn_ref(t[0], t[1], t[2], torch.zeros_like(t[0]), 1, RELU)["z"], "bwd_bcast")
    gfull = (g / S).view(N, 1, C).expand(N, S, C)
    ref, sc = _gn_ref(x, gm, bt, gfull, 1, RELU), _gn_scales(x, gm, bt, gfull, 1, RELU)
    _assert_relu_safe(ref["z"], "bwd_bcast")
    xd, gd, bd = x.to(DEV).to(dtype), gm.to(DEV), bt.to(DEV)
    y, mean, rstd = torch.empty_like(xd), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    lib("hdmoe_groupnorm_fwd", y, mean, rstd, xd, gd, bd, N, S, C, 1, RELU, EPS, _dt(dtype))
    dx = torch.full_like(xd, float("nan"))
    dg, db, ws = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.full((2 * N,), float("nan"), device=DEV)
    lib("hdmoe_groupnorm_bwd_bcast", dx, dg, db, ws, g.to(DEV), 1.0 / S, xd, gd, bd, mean, rstd, N, S, C, 1, RELU, _dt(dtype))
    _match(y, ref["y"], _bound(ref["y"], sc["y"], K_Y, dtype), "bwd_bcast: y")
    _match(dx, ref["dx"], _bound(ref["dx"], sc["dx"], K_DX, dtype), "bwd_bcast: dx")
    _match(dg, ref["dg"], _bound(ref["dg"], sc["dg"], K_SUM), "bwd_bcast: dgamma")
    _match(db, ref["db"], _bound(ref["db"], sc["db"], K_SUM), "bwd_bcast: dbeta")


@pytest.mark.parametrize("C,G", [(24, 3), (256, 128), (4100, 1)])
def test_group_norm_rejects_bad_arguments(lib, C, G):
    N, S = 1, 2
    x = torch.ones(N, S, C, device=DEV)
    y = torch.full_like(x, 7.0)
    gm, bt = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    mean, rstd, ws = torch.empty(N * G, device=DEV), torch.empty(N * G, device=DEV), torch.zeros(2 * N * G, device=DEV)
    with pytest.raises(RuntimeError):
        lib("hdmoe_groupnorm_fwd", y, mean, rstd, x, gm, bt, N, S, C, G, NONE, EPS, 0)
    with pytest.raises(RuntimeError):
        lib("hdmoe_groupnorm_bwd", y, gm.clone(), bt.clone(), ws, x, x, gm, bt, mean, rstd, N, S, C, G, NONE, 0)
    assert bool((y == 7.0).all())                            # nothing was launched


@pytest.mark.parametrize("S,C,G,act", [(33, 32, 8, SILU), (1023, 32, 4, NONE)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_batch_independent(dtype, S, C, G, act):
    """ops._gn_parts: the forward's summation order is a function of S only -- sample 0 of a 3-sample batch keeps every bit alone."""
    x, gm, bt, _ = _gn_make(3, S, C, G, act, dtype, 71)
    xd, gd, bd = x.to(DEV).to(dtype), gm.to(DEV), bt.to(DEV)
    y3 = _ops().group_norm(xd, gd, bd, G, act, EPS)
    y1 = _ops().group_norm(xd[:1].clone(), gd, bd, G, act, EPS)
    assert torch.equal(y3[0], y1[0])


# =====================================================================================================
# 3. router-trunk family: GroupNorm(1, C) + ReLU folded into the neighbouring kernels (direct calls; the ReLU is always on)
# =====================================================================================================
def _trunk_make(N, S, C, seed, CI=None):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                  # noqa: E731
    t = dict(y=r(N, S, C) * 1.7 + 0.4, gamma=1 + 0.3 * r(C), beta=0.2 * r(C), g=r(N, C) + 0.25, dz=_rnd(r(N, S, C) + 0.25, torch.bfloat16))
    if CI is not None:
        t.update(xin=r(N, S, CI) * 1.3 - 0.1, isc=1 + 0.2 * r(N, CI), ish=0.3 * r(N, CI))
    yd = t["y"].double().reshape(N, -1)
    t["mean"] = yd.mean(1).float()
    t["rstd"] = (yd.var(1, unbiased=False) + EPS).rsqrt().float()
    return t


def _trunk_z(t):
    return _gn1_ref(t["y"], t["gamma"], t["beta"], t["mean"], t["rstd"])["z"]


def _trunk_inputs(N, S, C, base_seed, CI=None, extra_z=None):
    assert N * S * max(C, CI or 0) <= 44000
    zof = _trunk_z if extra_z is None else (lambda t: torch.cat([_trunk_z(t).reshape(-1), extra_z(t).reshape(-1)]))
    return _relu_safe(lambda s: _trunk_make(N, S, C, base_seed + 1000 * s, CI), zof, f"trunk {(N, S, C, CI)}")


def _slots_of(y, slots):
    """(N, slots, 2) fp32 partial (sum, sum of squares) of y (N, S, C): each sample's elements cut into `slots` chunks (empty ones give 0)."""
    flat = y.double().reshape(y.shape[0], -1)
    ch = torch.tensor_split(flat, slots, dim=1)
    return torch.stack([torch.stack([c.sum(1), c.square().sum(1)], -1) for c in ch], 1).float().contiguous()


# (N, slots, S, C): slots on both sides of the 64 lanes; rows = 1024 / (C / 4) = 1024, 170 (1020 of 1024 threads), 32, 4; S below and above
# rows, through the 4-way unrolled loop (S > 3 rows) and its tail
FIN_CASES = [(3, 1, 1, 4), (2, 65, 700, 4), (2, 64, 170, 4), (2, 64, 3, 24), (2, 65, 170, 24), (2, 130, 700, 24), (2, 1, 170, 128),
             (2, 130, 1, 128), (1, 130, 3, 1024), (1, 64, 37, 1024)]


def _fin_ref(ws, count):
    s = ws.double().sum(1)
    m = s[:, 0] / count
    ex2 = s[:, 1] / count
    var = (ex2 - m * m).clamp_min(0.0)
    rs = (var + EPS).rsqrt()
    rel = 1.0 + ex2 / (var + EPS)
    return m, rs, ex2, rel


def _check_finalize(tag, mean, rstd, scale, shift, ws, count, gm, bt):
    m, rs, ex2, rel = _fin_ref(ws, count)
    _match(mean, m, _bound(m, ex2.sqrt(), K_STAT), f"{tag}: mean", zeros=False)
    _match(rstd, rs, K_STAT * U * rs * rel, f"{tag}: rstd")
    g64, b64 = gm.double(), bt.double()
    sc = rs[:, None] * g64
    _match(scale, sc, K_STAT * U * sc.abs() * rel[:, None], f"{tag}: scale")
    sh = b64 - m[:, None] * sc
    _match(shift, sh, K_STAT * U * (b64.abs() + (m.abs() + ex2.sqrt())[:, None] * sc.abs() * rel[:, None]), f"{tag}: shift")


@pytest.mark.parametrize("N,slots,S,C", FIN_CASES, ids=["-".join(map(str, c)) for c in FIN_CASES])
def test_gn1_finalize_and_pool(lib, N, slots, S, C):
    """hdmoe_gn1_finalize, hdmoe_gn1_relu_mean, hdmoe_gn1_finalize_relu_mean and hdmoe_gn1_finalize_relu_mean_pq on the same inputs."""
    t = _trunk_inputs(N, S, C, 81 + slots + S)
    y, gm, bt = t["y"], t["gamma"], t["beta"]
    ws = _slots_of(y, slots)
    _assert_relu_safe(_trunk_z(t), "gn1 pool")
    dev = {k: v.to(DEV) for k, v in dict(y=y, gm=gm, bt=bt, ws=ws).items()}
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)                       # noqa: E731
    tag = f"gn1 {(N, slots, S, C)}"
    # finalize alone
    sc, sh, mean, rstd = nan(N, C), nan(N, C), nan(N), nan(N)
    lib("hdmoe_gn1_finalize", sc, sh, mean, rstd, dev["ws"], dev["gm"], dev["bt"], N, slots, C, S * C, EPS)
    _check_finalize(tag + " finalize", mean, rstd, sc, sh, ws, S * C, gm, bt)
    # the pool over given scale / shift: the reference uses the same fp32 scale / shift
    out = nan(N, C)
    lib("hdmoe_gn1_relu_mean", out, dev["y"], sc, sh, N, S, C)
    sc64, sh64 = sc.cpu().double()[:, None, :], sh.cpu().double()[:, None, :]
    z = y.double() * sc64 + sh64
    _assert_relu_safe(z, tag + " relu_mean")
    _match(out, F.relu(z).mean(1), _bound(F.relu(z).mean(1), 1.0 + float((y.double() * sc64).abs().max()), K_Y), f"{tag} relu_mean: out")
    # the fused forms: statistics as above; out / pcnt / qsum against fp64 under the fp32 mean / rstd the kernel itself wrote
    for pq in (False, True):
        out, sc2, sh2, mean2, rstd2, P, Q = nan(N, C), nan(N, C), nan(N, C), nan(N), nan(N), nan(N, C), nan(N, C)
        if pq:
            lib("hdmoe_gn1_finalize_relu_mean_pq", out, sc2, sh2, mean2, rstd2, P, Q, dev["y"], dev["ws"], dev["gm"], dev["bt"], N, slots, S, C, EPS)
        else:
            lib("hdmoe_gn1_finalize_relu_mean", out, sc2, sh2, mean2, rstd2, dev["y"], dev["ws"], dev["gm"], dev["bt"], N, slots, S, C, EPS)
        name = f"{tag} finalize_relu_mean{'_pq' if pq else ''}"
        _check_finalize(name, mean2, rstd2, sc2, sh2, ws, S * C, gm, bt)
        assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and torch.equal(sc2, sc) and torch.equal(sh2, sh), name
        ref = _gn1_ref(y, gm, bt, mean2.cpu(), rstd2.cpu())
        _assert_relu_safe(ref["z"], name)
        _match(out, ref["pooled"], _bound(ref["pooled"], 1.0 + float(ref["z"].abs().max()), K_Y), f"{name}: out")
        if pq:
            assert torch.equal(P.cpu().double(), ref["pcnt"]), f"{name}: pcnt"
            _match(Q, ref["qsum"], _bound(ref["qsum"], ref["sc_q"], K_SUM), f"{name}: qsum")


def test_gn1_constant_sample_clamps_the_variance(lib):
    """A sample with constant y: E[y^2] - mean^2 comes out at -0.25 delta < 0 (delta = the rounding of the fp32 1 / count, upwards for this
    count), the clamp makes it 0, rstd = eps^-1/2 and everything stays finite."""
    N, S, C, slots = 2, 3, 24, 5
    count = S * C
    assert float(torch.tensor(1.0) / torch.tensor(float(count))) > 1.0 / count
    t = _trunk_make(N, S, C, 91)
    t["y"][0] = 0.5
    y, gm, bt = t["y"], t["gamma"], t["beta"]
    assert float(bt.abs().min()) > 1e-3                      # z = beta for the constant sample: away from the ReLU's edge
    ws = _slots_of(y, slots)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)                       # noqa: E731
    out, sc, sh, mean, rstd, P, Q = nan(N, C), nan(N, C), nan(N, C), nan(N), nan(N), nan(N, C), nan(N, C)
    lib("hdmoe_gn1_finalize_relu_mean_pq", out, sc, sh, mean, rstd, P, Q, y.to(DEV), ws.to(DEV), gm.to(DEV), bt.to(DEV), N, slots, S, C, EPS)
    sc1, sh1, mean1, rstd1 = nan(N, C), nan(N, C), nan(N), nan(N)
    lib("hdmoe_gn1_finalize", sc1, sh1, mean1, rstd1, ws.to(DEV), gm.to(DEV), bt.to(DEV), N, slots, C, count, EPS)
    for r_, m_, what in ((rstd, mean, "fused"), (rstd1, mean1, "finalize")):
        r0 = float(r_[0])
        assert abs(r0 - EPS ** -0.5) <= K_STAT * U * EPS ** -0.5, (what, r0)
        assert abs(float(m_[0]) - 0.5) <= K_STAT * U * 0.5, (what, float(m_[0]))
    for v in (out, sc, sh, P, Q, sc1, sh1):
        assert bool(torch.isfinite(v).all())
    # z = (0.5 - mean) rstd gamma + beta: |0.5 - mean| <= u, so out = relu(beta) within u rstd |gamma| (+ the rounding of the sum)
    want = F.relu(bt.double())
    _match(out[0], want, K_Y * U * (want + 1.0 + 0.5 * EPS ** -0.5 * gm.double().abs()), "constant sample: out", zeros=False)
    assert torch.equal(P[0].cpu(), (bt > 0).float() * S)


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("C", [8, 24])
def test_gn1t_act(lib, C, with_scale):
    N, S = 2, 19

    def make(seed):
        gen = _gen(95 + C + 1000 * seed)
        r = lambda *s: torch.randn(*s, generator=gen)                              # noqa: E731
        return r(N, S, C) * 1.3 - 0.1, 1 + 0.2 * r(N, C), 0.3 * r(N, C)
    zof = lambda t: t[0].double() * t[1].double()[:, None] + t[2].double()[:, None]          # noqa: E731
    y, sc, sh = _relu_safe(make, zof, "gn1t_act")
    out = torch.full((N, S, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    if with_scale:
        z = zof((y, sc, sh))
        _assert_relu_safe(z, "gn1t_act")
        lib("hdmoe_gn1t_act", out, y.to(DEV), sc.to(DEV), sh.to(DEV), N, S, C)
        ref = F.relu(z)
        _match(out, ref, _bound(ref, 1.0 + float(z.abs().max()), K_Y, torch.bfloat16), f"gn1t_act C={C}")
    else:
        lib("hdmoe_gn1t_act", out, y.to(DEV), None, None, N, S, C)
        assert torch.equal(out.cpu(), y.to(torch.bfloat16)), f"gn1t_act C={C}: a plain fp32 -> bf16 conversion"
    with pytest.raises(RuntimeError):
        lib("hdmoe_gn1t_act", out, y.to(DEV), sc.to(DEV), None, N, S, C)


def _check_trunk_bwd(tag, ref, dx, dg, db, pre_g, pre_b, s1=None, s2=None):
    _match(dx, ref["dx"], _bound(ref["dx"], ref["sc_dx"], K_DX, torch.bfloat16), f"{tag}: dx")
    _match(dg, pre_g.double() + ref["dg"], _bound(ref["dg"], ref["sc_dg"] + pre_g.double().abs(), K_SUM), f"{tag}: dgamma", zeros=False)
    _match(db, pre_b.double() + ref["db"], _bound(ref["db"], ref["sc_db"] + pre_b.double().abs(), K_SUM), f"{tag}: dbeta", zeros=False)
    if s1 is not None:
        _match(s1, ref["s1"], _bound(ref["s1"], ref["sc_s1"], K_SUM), f"{tag}: s1", zeros=False)
        _match(s2, ref["s2"], _bound(ref["s2"], ref["sc_s2"], K_SUM), f"{tag}: s2", zeros=False)


@pytest.mark.parametrize("form", ["dz", "g"])
@pytest.mark.parametrize("N,S,C", [(3, 50, 4), (2, 37, 64), (1, 5, 2048)])
def test_gn1t_bwd(lib, N, S, C, form):
    """hdmoe_gn1t_bwd: C = 4 is a single 4-channel vector per row, C = 2048 fills the 512-thread block with one row."""
    t = _trunk_inputs(N, S, C, 101 + C)
    dz, g, gs = (t["dz"], None, 1.0) if form == "dz" else (None, t["g"], 1.0 / S)
    ref = _gn1_ref(t["y"], t["gamma"], t["beta"], t["mean"], t["rstd"], dz, g, gs)
    _assert_relu_safe(ref["z"], "gn1t_bwd")
    d = {k: v.to(DEV) for k, v in t.items()}
    dx = torch.full((N, S, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    pre_g, pre_b = 0.5 + torch.arange(C).float() / C, -0.25 - torch.arange(C).float() / C
    dg, db, ws = pre_g.to(DEV), pre_b.to(DEV), torch.full((2 * N,), float("nan"), device=DEV)
    lib("hdmoe_gn1t_bwd", dx, dg, db, ws, None if dz is None else d["dz"].to(torch.bfloat16), None if g is None else d["g"], gs,
        d["y"], d["gamma"], d["beta"], d["mean"], d["rstd"], N, S, C)
    _check_trunk_bwd(f"gn1t_bwd {(N, S, C)} {form}", ref, dx, dg, db, pre_g, pre_b, ws[:N], ws[N:])


# (N, S, C, CI)
GN1T_CASES = [
    (1, 1, 8, 8),                # one row, one vector
    (3, 15, 24, 40),             # C / 8 = 3 and CI / 8 = 5 do not divide 256: idle tail threads; S < 16: one row range per sample
    (2, 127, 16, 8), (2, 128, 16, 8), (2, 129, 16, 8),       # gn1t_parts = 1 (S < 128 and S / 128 = 1); row ranges of apply: 7, 8, 8
    (1, 2049, 8, 16),            # gn1t_parts capped at 16 (129 rows each, the last 114)
    (65, 17, 24, 24),            # N > 64: the channel blocks' lane loop runs twice
    (1, 2, 2048, 8),             # one row per pass of the block, two rows in flight
    (2, 300, 16, 8),             # gn1t_parts = 2
]


@pytest.mark.parametrize("form", ["dz", "pooled"])
@pytest.mark.parametrize("N,S,C,CI", GN1T_CASES, ids=["-".join(map(str, c)) for c in GN1T_CASES])
def test_gn1t_stats_and_apply(lib, N, S, C, CI, form):
    import hdmoe_hip
    with_scale = (N, S, C, CI) != (2, 128, 16, 8)            # one case with a = bf16(xin)
    za = (lambda t: t["xin"].double() * t["isc"].double()[:, None] + t["ish"].double()[:, None]) if with_scale else None
    t = _trunk_inputs(N, S, C, 111 + S + C, CI, za)
    ref0 = _gn1_ref(t["y"], t["gamma"], t["beta"], t["mean"], t["rstd"])
    _assert_relu_safe(ref0["z"], "gn1t")
    pooled = form == "pooled"
    pcnt, qsum = ref0["pcnt"].float(), ref0["qsum"].float()
    dz, g, gs = (None, t["g"], 1.0 / S) if pooled else (t["dz"], None, 1.0)
    ref = _gn1_ref(t["y"], t["gamma"], t["beta"], t["mean"], t["rstd"], dz, g, gs)
    if pooled:      # the kernel forms s1 / s2 / dgamma / dbeta from the fp32 pcnt / qsum it is given: so does the reference
        k = (t["g"].double() * gs)
        gm = t["gamma"].double()
        ref["s1"], ref["s2"] = (k * gm * pcnt.double()).sum(1), (k * gm * qsum.double()).sum(1)
        ref["dg"], ref["db"] = (k * qsum.double()).sum(0), (k * pcnt.double()).sum(0)
        ref["sc_dg"], ref["sc_db"] = (k * qsum.double()).abs().sum(0), (k * pcnt.double()).abs().sum(0)
        N_, m_, rs_ = N, t["mean"].double().view(N, 1, 1), t["rstd"].double().view(N, 1, 1)
        dzz = (k.view(N_, 1, C).expand(N_, S, C)) * (ref["z"] > 0)
        ref["dx"] = rs_ * (dzz * gm - (ref["s1"].view(N, 1, 1) + ref["xh"] * ref["s2"].view(N, 1, 1)) / (S * C))
        # s1 / s2 are sums of up to C products whose factors pcnt (<= S) and qsum carry the magnitude: their rounding reaches dx
        ref["sc_dx"] = ref["sc_dx"] + rs_.abs() * ((k * gm * pcnt.double()).abs().amax(1).view(N, 1, 1)
                                                   + ref["xh"].abs() * (k * gm * qsum.double()).abs().amax(1).view(N, 1, 1)) / (S * C)
    d = {k_: v.to(DEV) for k_, v in t.items()}
    dzd = d["dz"].to(torch.bfloat16)
    dx = torch.full((N, S, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    a = torch.full((N, S, CI), float("nan"), dtype=torch.bfloat16, device=DEV)
    pre_g, pre_b = 0.5 + torch.arange(C).float() / C, -0.25 - torch.arange(C).float() / C
    dg, db = pre_g.to(DEV), pre_b.to(DEV)
    ws = None
    if not pooled:
        nf = hdmoe_hip.lib().hdmoe_gn1t_stats_floats(N, S, C)
        parts = max(1, min(16, S // 128))
        assert nf == 2 * N * parts * (1 + C)
        ws = torch.full((nf,), float("nan"), device=DEV)      # an unwritten slot shows up as NaN
        lib("hdmoe_gn1t_stats", ws, dzd, d["y"], d["gamma"], d["beta"], d["mean"], d["rstd"], N, S, C)
        assert bool(torch.isfinite(ws).all()), "gn1t_stats left a slot unwritten"
        slots = ws[:2 * N * parts].view(N, parts, 2).cpu().double().sum(1)
        tag = f"gn1t_stats {(N, S, C)}"
        _match(slots[:, 0], ref["s1"], _bound(ref["s1"], ref["sc_s1"], K_SUM), f"{tag}: s1", zeros=False)
        _match(slots[:, 1], ref["s2"], _bound(ref["s2"], ref["sc_s2"], K_SUM), f"{tag}: s2", zeros=False)
        wsc = ws[2 * N * parts:].view(2, C, N * parts).cpu().double().sum(-1)
        _match(wsc[0], ref["dg"], _bound(ref["dg"], ref["sc_dg"], K_SUM), f"{tag}: dgamma slots", zeros=False)
        _match(wsc[1], ref["db"], _bound(ref["db"], ref["sc_db"], K_SUM), f"{tag}: dbeta slots", zeros=False)
    lib("hdmoe_gn1t_apply", dx, a, dg, db, ws, None if pooled else dzd, d["g"] if pooled else None, gs, pcnt.to(DEV) if pooled else None,
        qsum.to(DEV) if pooled else None, d["y"], d["gamma"], d["beta"], d["mean"], d["rstd"], d["xin"], d["isc"] if with_scale else None,
        d["ish"] if with_scale else None, N, S, C, CI)
    tag = f"gn1t_apply {(N, S, C, CI)} {form}"
    _check_trunk_bwd(tag, ref, dx, dg, db, pre_g, pre_b)
    if with_scale:
        z = za(t)
        _match(a, F.relu(z), _bound(F.relu(z), 1.0 + float(z.abs().max()), K_Y, torch.bfloat16), f"{tag}: a")
    else:
        assert torch.equal(a.cpu(), t["xin"].to(torch.bfloat16)), f"{tag}: a = bf16(xin)"


# =====================================================================================================
# calibration (CPU only; `PYTHONPATH=. python tests/test_norm_kernels.py`): worst |fp32 torch - fp64| / (u (|r| + scale)) per quantity
# =====================================================================================================
def _calibrate():
    worst = {}

    def note(fam, kind, a, r, scale):
        den = U * (r.abs() + scale)
        ok = den > 0
        ratio = float(((a.double() - r).abs()[ok] / den[ok]).max()) if ok.any() else 0.0
        assert fam.startswith("group_norm, F.") or bool(((a.double() - r)[~ok] == 0).all())
        worst[(kind, fam)] = max(worst.get((kind, fam), 0.0), ratio)

    f32 = torch.float32
    for dtype in (torch.float32, torch.bfloat16):
        rowcases = [(r, C, dtype, 100 + C, {}) for r in (1, 70) for C in ROW_CS] + [(70, C, dtype, 5, dict(mean=100.0, std=1.0)) for C in (256, 30)]
        rowcases += [(r, C, dt, 7, {}) for (r, C, dt) in LONG_ROWS if dt == dtype]
        for rows, C, dt, seed, kw in rowcases:
            x, gm, bt, g = _ln_inputs(rows, C, dt, seed, **kw)
            r64, t32, sc = _ln_ref(x, gm, bt, g), _ln_ref(x, gm, bt, g, f32), _ln_scales(x, gm, bt, g)
            r32 = _gn_formula(x.unsqueeze(1), gm, bt, g.unsqueeze(1), 1, NONE, f32)
            for key, kind in (("y", "y"), ("dx", "dx"), ("dg", "sum"), ("db", "sum")):
                note("layer_norm, centred formulas", kind, r32[key].reshape(r64[key].shape), r64[key], sc[key])
                note("layer_norm, F.layer_norm", kind, t32[key], r64[key], sc[key])
            if kw:
                continue
            x, dxn, dh = _pn_inputs(rows, C, dt, 300 + C)
            r64, r32, sc = _pn_ref(x, dxn, dh, 0.3), _pn_ref(x, dxn, dh, 0.3, f32), _pn_scales(x, dxn, dh, 0.3)
            for key, kind in (("xn", "y"), ("h", "y"), ("dx", "dx")):
                note("pixel_norm", kind, r32[key], r64[key], sc["y" if kind == "y" else "dx"])
        for C in (3, 8, 24, 256):
            x, dxn, dh = _pn_edge_rows(C, dtype, 400 + C)
            r64, r32, sc = _pn_ref(x, dxn, dh, 0.3), _pn_ref(x, dxn, dh, 0.3, f32), _pn_scales(x, dxn, dh, 0.3)
            for key, kind in (("xn", "y"), ("h", "y"), ("dx", "dx")):
                note("pixel_norm", kind, r32[key], r64[key], sc["y" if kind == "y" else "dx"])
        gncases = [(c, 31 + c[1] + c[2], {}) for c in GN_CASES] + [((2, 300, 16, 2, NONE), 41, dict(mean=100.0, std=1.0)), ((2, 130, 16, 2, SILU), 53, {})]
        for (N, S, C, G, act), seed, kw in gncases:
            x, gm, bt, g = _gn_inputs(N, S, C, G, act, dtype, seed, **kw)
            r64, t32, sc = _gn_ref(x, gm, bt, g, G, act), _gn_ref(x, gm, bt, g, G, act, f32), _gn_scales(x, gm, bt, g, G, act)
            r32 = _gn_formula(x, gm, bt, g, G, act, f32)
            for key, kind in (("y", "y"), ("dx", "dx"), ("dg", "sum"), ("db", "sum")):
                note("group_norm, centred formulas", kind, r32[key], r64[key], sc[key])
                note("group_norm, F.group_norm", kind, t32[key], r64[key], sc[key])
            m, rs, bm, brs = _stat_bounds(x, G)
            note("group_norm", "stat", r32["mean"], m, bm / (K_STAT * U) - m.abs())
            note("group_norm", "stat", r32["rstd"], rs, brs / (K_STAT * U) - rs.abs())
    trunk = [(N, S, C, None, 81 + sl + S) for (N, sl, S, C) in FIN_CASES] + [(N, S, C, None, 101 + C) for (N, S, C) in ((3, 50, 4), (2, 37, 64), (1, 5, 2048))]
    trunk += [(N, S, C, CI, 111 + S + C) for (N, S, C, CI) in GN1T_CASES]
    for N, S, C, CI, seed in trunk:
        t = _trunk_inputs(N, S, C, seed, CI)
        for dz, g, gs in ((t["dz"], None, 1.0), (None, t["g"], 1.0 / S)):
            r64 = _gn1_ref(t["y"], t["gamma"], t["beta"], t["mean"], t["rstd"], dz, g, gs)
            r32 = _gn1_ref(t["y"], t["gamma"], t["beta"], t["mean"], t["rstd"], dz, g, gs, ft=f32)
            note("gn1", "y", r32["pooled"], r64["pooled"], 1.0 + float(r64["z"].abs().max()))
            note("gn1", "sum", r32["qsum"], r64["qsum"], r64["sc_q"])
            note("gn1", "dx", r32["dx"], r64["dx"], r64["sc_dx"])
            for key in ("s1", "s2", "dg", "db"):
                note("gn1", "sum", r32[key], r64[key], r64["sc_" + key])
        yf = t["y"].reshape(N, -1)
        m, var, ex2 = yf.double().mean(1), yf.double().var(1, unbiased=False), yf.double().square().mean(1)
        m32 = yf.mean(1)
        v32 = (yf.square().mean(1) - m32 * m32).clamp_min(0.0)                      # the finalize's one-pass form, in fp32
        note("gn1", "stat", m32, m, ex2.sqrt())
        note("gn1", "stat", (v32 + EPS).rsqrt(), (var + EPS).rsqrt(), (var + EPS).rsqrt() * (1.0 + ex2 / (var + EPS)))
    for (kind, fam), v in sorted(worst.items()):
        print(f"{kind:5s} {fam:32s} worst fp32-CPU ratio {v:9.3f}")
    for kind in ("y", "dx", "sum", "stat"):
        v = max(r for (k, fam), r in worst.items() if k == kind and not fam.endswith(("F.layer_norm", "F.group_norm")))
        print(f"{kind:5s} worst {v:.3f} -> K = {2.0 ** math.ceil(math.log2(4 * v)):.0f}")


if __name__ == "__main__":
    _calibrate()
