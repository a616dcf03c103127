"""The pointwise, broadcast and reduce kernels of csrc/elementwise.hip against float64 on the CPU, on every arm of their host-side dispatch.

Reference.  Inputs are drawn from a seed and rounded to the case's dtype; float scalars are rounded to fp32 (what the C ABI passes).  The
truth is those values evaluated in float64 on the CPU: oracle.mp_silu / oracle.mp_cat / oracle.resample with autograd where the oracle has
the operation, F.conv2d / F.conv_transpose2d for the FIR, and a few lines that restate the formula of the kernel comment for the rest.
Kernels that take an earlier result as an input (sigmoid_bwd's y, softmax_rows_bwd's y, gate_mix_bwd's gate) get the float64 result rounded
to the input's dtype, and the reference uses those same rounded values.  hdmoe_cat2_silu_fwd promises that mp_silu sees the stored
concatenation, so out_h is compared with float64 mp_silu of the kernel's own `out` (which is itself compared with the truth).

Bounds.  u = 2**-24.  An output k must satisfy |k - r| <= K u (|r| + scale) + under; a bf16 output adds 2**-8 |r|.  scale = the largest
magnitude the quantity passes through before any cancellation:
  pointwise   the sum of the magnitudes of the terms of the formula (a x + b y: |a x| + |b y|; a product: |r|)
  activation  s = sigmoid(z), amp = 1 + |z| (1 - s): __expf(-z) is exp2(-z log2 e), and the rounding of that product is a relative error
              of |z| u in exp(-z), (1 - s) |z| u in s.  mp_silu: |z| s amp / 0.596; mp_silu' = s (1 + z (1 - s)) / 0.596:
              |dy| s (1 + |z|) amp / 0.596, its two terms by magnitude with 1 - s taken at the 1 it is cancelled from (fp32 forms 1 - s
              with an absolute error of u, which z multiplies: 16 u at z = 16, in the CPU's fp32 as in the kernel), times the same
              amplification; sigmoid(a x): s (1 + 2 |z| (1 - s)) (the product a x is rounded, too)
  reduction   the sum of the magnitudes of the terms, plus the magnitude of what the kernel adds into
  softmax     p_i (1 + |d_i| + sum_j p_j |d_j|), d = x - max (each exponent's argument error is |d| u); 2-way gate: g_i (1 + (1 - g_i) |l0 - l1|);
              what is built on a gate (out, dlogits) carries these through its own terms taken by magnitude
under = 2**-126, the smallest normal fp32: an output below it may be flushed to zero (every class), and in the activation and softmax /
gate classes 2**-126 times the sensitivity of the output to the intermediate that underflows is added: v_exp_f32 / v_rcp_f32 flush
denormal results, and exp(89) already exceeds fp32, so sigmoid(-89) = 2.2e-39 comes out as 0 and mp_silu(-89) = -3.3e-37 as -0.  For
mp_silu that sensitivity is |x| / 0.596, for its gradient |dy| (1 + |x|) / 0.596, for a softmax its scale factor.
Zero and non-finite patterns: wherever the reference is exactly zero or non-finite the kernel must be, too.  Every output buffer is filled
with NaN (or the value the kernel must add to / keep) and has 8 guard elements on either side, which must still hold their fill afterwards.

K is four times the worst ratio |fp32 CPU - fp64| / (u (|r| + scale) + under) that `_calibrate` measured over every case table of this
file (`PYTHONPATH=. python tests/test_elementwise_kernels.py`, CPU only, never run by a test), rounded up to a power of two; the factor of
four covers the kernels' other summation order and __expf / v_rcp_f32.
  class        worst fp32-CPU ratio (where)                                                       4 x worst   K
  pointwise    1.34  sigmoid_bwd, n = 1028, a = -2.5                                               5.34      8
  activation   2.72  film_silu du, C = 64, HW = 255, bf16 inputs                                  10.89     16
  reduction    1.97  sum_n, 16 sources of 1031 elements, src_scale given                           7.89      8
  softmax      1.94  gate_mix dlogits without dgate, 524,291 rows of 4 channels                    7.77      8
(hdmoe_cat2_silu_fwd has no table of its own: its `out` is the cat2 table's reference under the pointwise K, its out_h mp_silu under the
activation K.)
On the MI355X the kernels' own worst |error| / bound came out at 0.17 (pointwise), 0.91 (activation), 0.29 (reduction) and 0.62 (softmax)
for fp32 outputs.  The activation figure is film_silu at u e = -88: exp(88) is finite but 1 / (1 + exp(88)) = 5e-39 is denormal and
v_rcp_f32 returns 0, so the whole error is the `under` term; every other activation case stays below 0.5.  bf16 outputs reach
0.996: one rounding to 8 significant bits is the 2**-8 |r| part of their bound.

Which kernel each shape reaches (W = 4 fp32 / 8 bf16 elements per 16-byte vector; "vec" = the 16-byte arm, "scalar" = the one-element
arm.  axpby, mp_silu_fwd/bwd, scale_rows_fwd/bwd, cat2_fwd/bwd, pool2, upsample2, lerp_param_bwd, lerp_rows, known_blend and
film_silu_fwd are one body each: vec = op_kernel<T, W>, scalar = op_kernel<T, 1>.  film_silu_bwd, gate_mix_*, seq_reduce and the patch
relayouts keep a *_vec_kernel of their own beside the plain one.  The vector arm needs the count or channel count to divide by W and every
al16-tested pointer 16-byte aligned):
* sizes n in {1, W-1, W, W+1, 255, 257, 1024+W}: W and 1024+W -> vec, the rest scalar (axpby, mp_silu_fwd/bwd; known_blend:
  vec = known_blend_kernel<float, 4>, fp32 only, bf16 always known_blend_kernel<bf16, 1>; mp_silu_bwd_add has no scalar arm and takes {W, 1024+W};
  affine, mul, sigmoid_*, lerp_param_fwd, seq_bcast_add, bias_add, nchw_to_nhwc and the fp32 vector-path ops have one kernel).
  A view one element into a buffer, for each pointer in turn -> the scalar arm at a vec-eligible size.
* grid cap: n = 524,288 + 259 elements (scalar) and (524,288 + 3) W elements (vec): 2050 blocks wanted, grid_for caps at 2048, the
  grid-stride loop takes the rest.  cat2_fwd: 58,283 rows of (4, 5) channels / 18,079 rows of (14 W, 15 W) (29 vectors a row);
  scale_rows_fwd: 3 x 174,849 / 1 x 524,291 W; seq_bcast_add: 3 x 58,283 x 3; softmax_rows_fwd: 524,547 rows of 2; gate_mix_fwd:
  58,283 rows of 9 channels (scalar) / 524,291 rows of W (vec, lpr = 1).
* cat2_*: (W, W), (W, 3W), (3W, W) -> vec; (3, 5), (W, W+1) -> scalar; cat2_silu_* decline those two.
* pool2 / upsample2: C = W, 3W -> vec, C = 3 -> scalar; upsample2 runs at (Ho, Wo) = (2, 6) only, (1, 1) and (5, 4) are odd and declined.
  fir_resample: one kernel per direction (fir_down_kernel / fir_up_kernel).
* seq_reduce: C / W in {1, 2, 16, 256} -> seq_reduce_det_vec_kernel with R = 256, 128, 16, 1 row lanes (C / W = 256: the LDS tree runs
  zero times); C = 3W (256 % 3 != 0) and C = 5 -> seq_reduce_det_kernel (four partial sums: S = 1, 3 the tail loop only, 7, 9, 34 both).
  S = 0 (R - 1 at R = 1) is left out: an empty tensor has no pointer to pass.
* scale_rows_bwd: L = W, 8192, 8192 + W, 2048 W + W -> vec (one chunk of 2048 vectors; fp32 8192 = exactly one chunk and 8196 = one vector
  into the second; bf16 8192 and 8200 inside the first, 16,392 one vector into the second); L = 8193 -> scalar, one element into its
  second chunk of 8192.  Chunks meet in ds through atomicAdd.
* bias_add / colsum: rows 1, 63, 64, 65, 130 -> 1, 1, 1, 2, 3 row chunks of 64; L = 1, 255, 257 -> 1, 1, 2 column blocks.
* film_silu: C / W in {1, 8, 256} -> vec forward and backward; C = 3W -> vec forward, scalar backward (256 % 3 != 0); C = 5 -> scalar
  both.  HW = 1, 255, 256 -> one 256-pixel workgroup per sample, 257 -> two, merged in de by atomicAdd.
* lerp_param_bwd: n = W, 1000 W, 262,145 W -> vec (1, 4, 1025 -> capped at 1024 blocks), n = 1001 -> scalar.
* gate_mix: C / W in {1, 2, 16, 64} -> vec (lpr lanes a row; rows lpr = 1, 2, 3, 6, 33, 48, 66, .. is not a multiple of 64 except where
  lpr = 64: the padded tail of the backward's shuffles); C / W = 3 (not a power of two), 65, 128 (> 64) and C = 5 -> scalar.
* 32-bit index overflow needs tensors above 2**31 elements and is not a test of a few seconds: out of scope here.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import hdmoe_oracle as O

gpu = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
TINY = 2.0 ** -126
K_PW, K_ACT, K_RED, K_SM = 8.0, 16.0, 8.0, 8.0
KS = dict(pointwise=K_PW, activation=K_ACT, reduction=K_RED, softmax=K_SM)
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
DIV = O.MP_SILU_DIV
GATE_K = float(torch.tensor(0.70710678118654752, dtype=F32))
CAP = 524288                                                 # grid_for: 2048 workgroups of 256 threads
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()
    from hdmoe_hip._lib import call
    yield call
    if _WORST:
        print("\nworst |err| / bound per class: " + ", ".join(f"{c} {v:.3f}" for c, v in sorted(_WORST.items())))


def _dt(dtype):
    return 0 if dtype == F32 else 1


def _W(dtype):
    return 4 if dtype == F32 else 8


def _f32(v):
    return float(torch.tensor(float(v), dtype=F32))


def _bound(r, scale, K, dtype=F32, under=0.0):
    b = K * U * (r.abs().nan_to_num(0.0) + scale) + under + TINY
    return b + (2.0 ** -8 * r.abs().nan_to_num(0.0) if dtype == BF16 else 0.0)


_WORST = {}                                                  # class -> the kernels' worst |err| / bound of this run


def _match(k, r, bound, msg, zeros=True, cls=None):
    """k (any float tensor) vs r (fp64 CPU): the same NaN and +-inf positions, exactly zero wherever r is exactly zero (zeros=False: r's
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
    if k_dtype == F32 and cls is not None:
        _WORST[cls] = max(_WORST.get(cls, 0.0), worst)
    print(f"{msg} [{str(k_dtype).replace('torch.', '')}]: worst |err| / bound = {worst:.3f}")
    assert not bad.any(), f"{msg}: {int(bad.sum())} entries over the bound, worst |err| {float(err[bad].max()):.3e} " \
                          f"at bound {float(b[bad][err[bad].argmax()]):.3e}"


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _rnd(t, dtype):
    return t.to(dtype).float()


def _dev(x, dtype, mis=False):
    """x (CPU, values already representable in dtype) on the device.  mis: a contiguous view that starts one element into a larger
    buffer, so its pointer is not 16-byte aligned."""
    if x is None:
        return None
    if not mis:
        return x.to(DEV).to(dtype).contiguous()
    base = torch.zeros(x.numel() + 8, dtype=dtype, device=DEV)
    base[1:1 + x.numel()] = x.to(DEV).to(dtype).reshape(-1)
    v = base[1:1 + x.numel()].view(x.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


_GUARDS = []


def _buf(shape, dtype, mis=False, fill=NAN):
    """An output buffer filled with `fill` (a float or a CPU tensor), 8 guard elements in front and 16 behind; mis: one element further in."""
    n = int(math.prod(shape))
    off = 8 + (1 if mis else 0)
    base = torch.full((n + 24,), NAN if torch.is_tensor(fill) else fill, dtype=dtype, device=DEV)
    if torch.is_tensor(fill):
        base[off:off + n] = fill.to(DEV).to(dtype).reshape(-1)
    v = base[off:off + n].view(shape)
    assert (v.data_ptr() % 16 != 0) == bool(mis)
    _GUARDS.append((base, off, n, NAN if torch.is_tensor(fill) else float(fill)))
    return v


def _guards_ok(msg):
    for base, off, n, fill in _GUARDS:
        g = torch.cat([base[:off], base[off + n:]])
        assert bool((g.isnan() if math.isnan(fill) else g == fill).all()), f"{msg}: a guard element was written"
    _GUARDS.clear()


def _raises_and_keeps(call, name, out, *args):
    """A decline: the status comes back before any launch, and the pre-filled output is unchanged."""
    before = out.clone()
    with pytest.raises(RuntimeError):
        call(name, *args)
    torch.cuda.synchronize()
    assert torch.equal(out, before), f"{name}: a declined call changed its output"


# =====================================================================================================
# shared pieces of the references
# =====================================================================================================
SPECIALS = [0.0, -0.0, -1.278, 20.0, -20.0, 89.0, -89.0, 100.0, -100.0]


def _act_x(gen, n, dtype, std=3.0):
    """Activation inputs: n values, the first min(n, 9) of them the special points (zeros, the cancellation point of mp_silu', large |x| on
    either side of where __expf overflows); no infinities."""
    x = torch.randn(n, generator=gen) * std
    k = min(n, len(SPECIALS))
    x[:k] = torch.tensor(SPECIALS[:k])
    return _rnd(x, dtype)


def _silu_sc(z):
    """(scale of mp_silu(z), scale of mp_silu'(z), underflow term of either) from fp64 z: see the module docstring."""
    z = z.double()
    s = torch.sigmoid(z)
    amp = 1.0 + z.abs() * (1.0 - s)
    return z.abs() * s * amp / DIV, s * (1.0 + z.abs()) * amp / DIV, TINY * z.abs() / DIV, TINY * (1.0 + z.abs()) / DIV


def _silu_and_grad(z, ft):
    """oracle.mp_silu(z) and mp_silu'(z) (autograd) in ft."""
    zr = z.detach().to(ft).clone().requires_grad_(True)
    h = O.mp_silu(zr)
    (g,) = torch.autograd.grad(h.sum(), zr)
    return h.detach(), g


def _pw_sizes(dtype):
    W = _W(dtype)
    return [1, W - 1, W, W + 1, 255, 257, 1024 + W]


def _cap_sizes(dtype):
    return [CAP + 259, (CAP + 3) * _W(dtype)]


class Fam:
    """One entry point (or a forward / backward pair): its case table, the reference in a given float type, the scales of the bounds and
    the launch.  cases(dtype) -> (tag, inputs); ref(inputs, ft) -> {key: r}; scl(inputs) -> {key: scale | (scale, under)};
    run(call, inputs, dtype, mis) -> {key: device tensor}; cls: {key: class}; ptrs: the pointers the host code tests with al16."""
    def __init__(self, name, cls, cases, ref, scl, run, ptrs=(), mis_case=None, dtypes=(F32, BF16), zeros=None):
        self.name, self.cls, self.cases, self.ref, self.scl, self.run = name, cls, cases, ref, scl, run
        self.ptrs, self.mis_case, self.dtypes, self.zeros = ptrs, mis_case, dtypes, zeros or {}


FAMS = {}


def _fam(*a, **kw):
    f = Fam(*a, **kw)
    FAMS[f.name] = f
    return f


def _split(sc):
    return sc if isinstance(sc, tuple) else (sc, 0.0)


def _check(fam, tag, got, inp, dtype):
    ref, sc = fam.ref(inp, torch.float64), fam.scl(inp)
    assert set(got) == set(ref), (tag, set(got), set(ref))
    for key, k in got.items():
        scale, under = _split(sc[key])
        c = fam.cls[key]
        _match(k, ref[key].double(), _bound(ref[key].double(), scale, KS[c], k.dtype, under), f"{fam.name} {tag}: {key}",
               zeros=fam.zeros.get(key, True), cls=c)


def _run_family(call, name, dtype):
    fam = FAMS[name]
    for tag, inp in fam.cases(dtype):
        got = fam.run(call, inp, dtype, ())
        torch.cuda.synchronize()
        _guards_ok(f"{name} {tag}")
        _check(fam, tag, got, inp, dtype)


def _run_misaligned(call, name, dtype):
    fam = FAMS[name]
    tag, inp = fam.mis_case(dtype)
    for p in fam.ptrs:
        got = fam.run(call, inp, dtype, (p,))
        torch.cuda.synchronize()
        _guards_ok(f"{name} {tag} {p} misaligned")
        _check(fam, f"{tag} {p} misaligned", got, inp, dtype)


# =====================================================================================================
# 1. generic pointwise: axpby, affine, mul, known_blend
# =====================================================================================================
def _axpby_cases(dtype):
    for n in _pw_sizes(dtype) + _cap_sizes(dtype):
        gen = _gen(1000 + n)
        x, y = _rnd(torch.randn(n, generator=gen), dtype), _rnd(torch.randn(n, generator=gen) * 2 + 0.5, dtype)
        for a, b, has_y in ((1.3, -0.7, True), (1.3, -0.7, False), (-0.6, 0.0, True)):
            yield f"n={n} a={a} b={b} y={'given' if has_y else 'null'}", dict(x=x, y=y if has_y else None, a=_f32(a), b=_f32(b))
            if n > CAP:
                break


def _axpby_ref(i, ft):
    r = i["a"] * i["x"].to(ft)
    return dict(out=r if i["y"] is None else r + i["b"] * i["y"].to(ft))


def _axpby_scl(i):
    s = abs(i["a"]) * i["x"].double().abs()
    return dict(out=s if i["y"] is None else s + abs(i["b"]) * i["y"].double().abs())


def _axpby_run(call, i, dtype, mis):
    x, y = _dev(i["x"], dtype, "x" in mis), _dev(i["y"], dtype, "y" in mis)
    out = _buf(x.shape, dtype, "out" in mis)
    call("hdmoe_axpby", out, x, y, i["a"], i["b"], x.numel(), _dt(dtype))
    return dict(out=out)


_fam("axpby", dict(out="pointwise"), _axpby_cases, _axpby_ref, _axpby_scl, _axpby_run, ptrs=("out", "x", "y"),
     mis_case=lambda dt: next(c for c in _axpby_cases(dt) if c[0].startswith(f"n={1024 + _W(dt)} ")))


def _affine_mul_cases(dtype):
    for n in _pw_sizes(dtype):
        gen = _gen(1100 + n)
        yield f"n={n}", dict(x=_rnd(torch.randn(n, generator=gen), dtype), y=_rnd(torch.randn(n, generator=gen) * 2 + 0.5, dtype),
                             a=_f32(-1.7), c=_f32(0.3))


def _affine_mul_run(call, i, dtype, mis):
    x, y = _dev(i["x"], dtype), _dev(i["y"], dtype)
    aff, mul = _buf(x.shape, dtype), _buf(x.shape, dtype)
    call("hdmoe_affine", aff, x, i["a"], i["c"], x.numel(), _dt(dtype))
    call("hdmoe_mul", mul, x, y, x.numel(), _dt(dtype))
    return dict(affine=aff, mul=mul)


_fam("affine_mul", dict(affine="pointwise", mul="pointwise"), _affine_mul_cases,
     lambda i, ft: dict(affine=i["a"] * i["x"].to(ft) + i["c"], mul=i["x"].to(ft) * i["y"].to(ft)),
     lambda i: dict(affine=abs(i["a"]) * i["x"].double().abs() + abs(i["c"]), mul=(i["x"].double() * i["y"].double()).abs()),
     _affine_mul_run)


def _blend_cases(dtype):
    for n in _pw_sizes(dtype):
        gen = _gen(1200 + n)
        r = lambda: _rnd(torch.randn(n, generator=gen), dtype)                     # noqa: E731
        m = torch.rand(n, generator=gen)
        m[0::3], m[1::5] = 0.0, 1.0                                                # hard mask values among the soft ones
        yield f"n={n}", dict(x=r(), x0=r(), nz=r(), m=m, s=_f32(2.5))


def _blend_ref(i, ft):
    k = i["m"].to(ft)
    return dict(x=k * (i["x0"].to(ft) + i["s"] * i["nz"].to(ft)) + (1.0 - k) * i["x"].to(ft))


def _blend_scl(i):
    k = i["m"].double()
    return dict(x=k * (i["x0"].double().abs() + abs(i["s"]) * i["nz"].double().abs()) + (1.0 - k).abs() * i["x"].double().abs())


def _blend_run(call, i, dtype, mis):
    x = _buf(i["x"].shape, dtype, "x" in mis, fill=i["x"])                        # in place
    call("hdmoe_known_blend", x, _dev(i["x0"], dtype, "x0" in mis), _dev(i["nz"], dtype, "noise" in mis), _dev(i["m"], F32, "mask" in mis),
         i["s"], x.numel(), _dt(dtype))
    return dict(x=x)


_fam("known_blend", dict(x="pointwise"), _blend_cases, _blend_ref, _blend_scl, _blend_run, ptrs=("x", "x0", "noise", "mask"),
     mis_case=lambda dt: next(c for c in _blend_cases(dt) if c[0] == f"n={1024 + _W(dt)}"))


# =====================================================================================================
# 2. activations: mp_silu_fwd / bwd / bwd_add, sigmoid_fwd / bwd
# =====================================================================================================
def _silu_cases(dtype):
    for n in _pw_sizes(dtype) + _cap_sizes(dtype):
        gen = _gen(2000 + n)
        yield f"n={n}", dict(x=_act_x(gen, n, dtype), dy=_rnd(torch.randn(n, generator=gen) + 0.25, dtype))


def _silu_ref(i, ft):
    h, g = _silu_and_grad(i["x"], ft)
    return dict(out=h, dx=i["dy"].to(ft) * g)


def _silu_scl(i):
    f, g, uf, ug = _silu_sc(i["x"])
    dy = i["dy"].double().abs()
    return dict(out=(f, uf), dx=(dy * g, dy * ug))


def _silu_run(call, i, dtype, mis):
    x, dy = _dev(i["x"], dtype, "x" in mis), _dev(i["dy"], dtype, "dy" in mis)
    out, dx = _buf(x.shape, dtype, "out" in mis), _buf(x.shape, dtype, "dx" in mis)
    call("hdmoe_mp_silu_fwd", out, x, x.numel(), _dt(dtype))
    call("hdmoe_mp_silu_bwd", dx, dy, x, x.numel(), _dt(dtype))
    return dict(out=out, dx=dx)


_fam("mp_silu", dict(out="activation", dx="activation"), _silu_cases, _silu_ref, _silu_scl, _silu_run, ptrs=("out", "x", "dx", "dy"),
     mis_case=lambda dt: next(c for c in _silu_cases(dt) if c[0] == f"n={1024 + _W(dt)}"))


def _silu_add_cases(dtype):
    W = _W(dtype)
    for n in (W, 1024 + W):
        for sx in (0.0, 0.7):
            gen = _gen(2100 + n)
            x = _act_x(gen, n, dtype) if n > W else _rnd(torch.tensor(SPECIALS[2:2 + W] if W == 4 else SPECIALS[1:9]), dtype)
            yield f"n={n} sx={sx}", dict(x=x, dy=_rnd(torch.randn(n, generator=gen) + 0.25, dtype), gx=_rnd(torch.randn(n, generator=gen), dtype),
                                         sx=_f32(sx))


def _silu_add_run(call, i, dtype, mis):
    x = _dev(i["x"], dtype)
    dx = _buf(x.shape, dtype)
    call("hdmoe_mp_silu_bwd_add", dx, _dev(i["dy"], dtype), x, _dev(i["gx"], dtype), i["sx"], x.numel(), _dt(dtype))
    return dict(dx=dx)


def _silu_add_scl(i):
    _, g, _, ug = _silu_sc(i["x"])
    dy = i["dy"].double().abs()
    return dict(dx=(abs(i["sx"]) * i["gx"].double().abs() + dy * g, dy * ug))


_fam("mp_silu_bwd_add", dict(dx="activation"), _silu_add_cases,
     lambda i, ft: dict(dx=i["sx"] * i["gx"].to(ft) + i["dy"].to(ft) * _silu_and_grad(i["x"], ft)[1]), _silu_add_scl, _silu_add_run)


def _sigmoid_cases(dtype):
    for n in _pw_sizes(dtype):
        for a in (1.0, -2.5):
            gen = _gen(2200 + n)
            x = _act_x(gen, n, dtype)
            y = _rnd(torch.sigmoid(_f32(a) * x.double()).float(), dtype)           # sigmoid_bwd's input: the stored forward result
            yield f"n={n} a={a}", dict(x=x, y=y, dy=_rnd(torch.randn(n, generator=gen) + 0.25, dtype), a=_f32(a))


def _sigmoid_ref(i, ft):
    y = i["y"].to(ft)
    return dict(out=torch.sigmoid(i["a"] * i["x"].to(ft)), dx=i["dy"].to(ft) * i["a"] * y * (1.0 - y))


def _sigmoid_scl(i):
    z = i["a"] * i["x"].double()
    s = torch.sigmoid(z)
    y = i["y"].double()
    return dict(out=(s * (1.0 + 2.0 * z.abs() * (1.0 - s)), TINY), dx=(i["dy"].double() * i["a"] * y * (1.0 - y)).abs())


def _sigmoid_run(call, i, dtype, mis):
    x = _dev(i["x"], dtype)
    out, dx = _buf(x.shape, dtype), _buf(x.shape, dtype)
    call("hdmoe_sigmoid_fwd", out, x, i["a"], x.numel(), _dt(dtype))
    call("hdmoe_sigmoid_bwd", dx, _dev(i["dy"], dtype), _dev(i["y"], dtype), i["a"], x.numel(), _dt(dtype))
    return dict(out=out, dx=dx)


_fam("sigmoid", dict(out="activation", dx="pointwise"), _sigmoid_cases, _sigmoid_ref, _sigmoid_scl, _sigmoid_run)


# =====================================================================================================
# 3. mp_cat: cat2_fwd / bwd, cat2_silu_fwd / bwd
# =====================================================================================================
CAT_T = 0.3                                                  # mp_cat's t: wa != wb even where Ca == Cb


def _cat_shapes(dtype):
    W = _W(dtype)
    return [(W, W), (W, 3 * W), (3 * W, W), (3, 5), (W, W + 1)]


def _cat_inputs(Ca, Cb, rows, dtype, seed):
    gen = _gen(seed)
    r = lambda *s: _rnd(torch.randn(*s, generator=gen) * 1.5, dtype)               # noqa: E731
    wa, wb = O.mp_cat_scales(Ca, Cb, CAT_T)
    i = dict(a=r(rows, Ca), b=r(rows, Cb), dout=r(rows, Ca + Cb), gh=r(rows, Ca + Cb), wa=_f32(wa), wb=_f32(wb), Ca=Ca, Cb=Cb, rows=rows)
    i["xcat"] = _rnd(torch.cat([i["a"], i["b"]], 1) * 2.0, dtype)
    return i


def _cat_cases(dtype):
    for Ca, Cb in _cat_shapes(dtype):
        for rows in (1, 7):
            yield f"Ca={Ca} Cb={Cb} rows={rows}", _cat_inputs(Ca, Cb, rows, dtype, 3000 + Ca + 7 * Cb + rows)
    W = _W(dtype)
    yield "grid cap, scalar", _cat_inputs(4, 5, (CAP + 259) // 9, dtype, 3001)
    yield "grid cap, vec", _cat_inputs(14 * W, 15 * W, (CAP + 3) // 29, dtype, 3002)


def _cat_ref(i, ft):
    a, b = (i[k].to(ft).clone().requires_grad_(True) for k in ("a", "b"))
    out = O.mp_cat(a, b, dim=1, t=CAT_T)
    da, db = torch.autograd.grad(out, (a, b), i["dout"].to(ft))
    return dict(out=out.detach(), da=da, db=db)


def _cat_scl(i):
    r = _cat_ref(i, torch.float64)
    return {k: v.abs() for k, v in r.items()}


def _cat_run(call, i, dtype, mis):
    a, b, dout = _dev(i["a"], dtype, "a" in mis), _dev(i["b"], dtype, "b" in mis), _dev(i["dout"], dtype, "dout" in mis)
    out, da, db = _buf(dout.shape, dtype, "out" in mis), _buf(a.shape, dtype, "da" in mis), _buf(b.shape, dtype, "db" in mis)
    call("hdmoe_cat2_fwd", out, a, b, i["wa"], i["wb"], i["Ca"], i["Cb"], i["rows"], _dt(dtype))
    call("hdmoe_cat2_bwd", da, db, dout, i["wa"], i["wb"], i["Ca"], i["Cb"], i["rows"], _dt(dtype))
    return dict(out=out, da=da, db=db)


_fam("cat2", dict(out="pointwise", da="pointwise", db="pointwise"), _cat_cases, _cat_ref, _cat_scl, _cat_run,
     ptrs=("out", "a", "b", "da", "db", "dout"), mis_case=lambda dt: ("Ca=W Cb=3W rows=7", _cat_inputs(_W(dt), 3 * _W(dt), 7, dt, 3003)))


def _cat_silu_cases(dtype):
    for Ca, Cb in _cat_shapes(dtype)[:3]:
        for rows in (1, 7):
            for gc in (True, False):
                i = _cat_inputs(Ca, Cb, rows, dtype, 3100 + Ca + 7 * Cb + rows)
                if rows == 7:                                # the special activation points, in both halves of the concatenation
                    i["xcat"][0, :4], i["xcat"][1, -4:] = _rnd(torch.tensor([-1.278, -89.0, 100.0, 0.0]), dtype), \
                        _rnd(torch.tensor([-100.0, 89.0, -0.0, 20.0]), dtype)
                i["gcat"] = i["dout"] if gc else None
                yield f"Ca={Ca} Cb={Cb} rows={rows} gcat={'given' if gc else 'null'}", i


def _cat_silu_bwd_ref(i, ft):
    """(da, db) = split((gcat + gh mp_silu'(xcat)) (wa | wb))"""
    g = i["gh"].to(ft) * _silu_and_grad(i["xcat"], ft)[1]
    if i["gcat"] is not None:
        g = g + i["gcat"].to(ft)
    return dict(da=g[:, :i["Ca"]] * i["wa"], db=g[:, i["Ca"]:] * i["wb"])


def _cat_silu_bwd_scl(i):
    _, gsc, _, ug = _silu_sc(i["xcat"])
    gh = i["gh"].double().abs()
    s, u = gh * gsc, gh * ug
    if i["gcat"] is not None:
        s = s + i["gcat"].double().abs()
    Ca, wa, wb = i["Ca"], abs(i["wa"]), abs(i["wb"])
    return dict(da=(s[:, :Ca] * wa, u[:, :Ca] * wa), db=(s[:, Ca:] * wb, u[:, Ca:] * wb))


def _cat_silu_bwd_run(call, i, dtype, mis):
    da, db = _buf(i["a"].shape, dtype), _buf(i["b"].shape, dtype)
    call("hdmoe_cat2_silu_bwd", da, db, _dev(i["gcat"], dtype), _dev(i["gh"], dtype), _dev(i["xcat"], dtype), i["wa"], i["wb"], i["Ca"], i["Cb"],
         i["rows"], _dt(dtype))
    return dict(da=da, db=db)


_fam("cat2_silu_bwd", dict(da="activation", db="activation"), _cat_silu_cases, _cat_silu_bwd_ref, _cat_silu_bwd_scl, _cat_silu_bwd_run)


# =====================================================================================================
# 4. resampling: pool2, upsample2, fir_resample
# =====================================================================================================
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _resample_cases(dtype):
    W = _W(dtype)
    for N in (1, 3):
        for Ho, Wo in ((1, 1), (2, 6), (5, 4)):
            for C in (W, 3 * W, 3):
                gen = _gen(4000 + 100 * N + 10 * Ho + C)
                i = dict(x=_rnd(torch.randn(N, 2 * Ho, 2 * Wo, C, generator=gen), dtype), N=N, Ho=Ho, Wo=Wo, C=C, scale=_f32(0.3), xs=None)
                if Ho % 2 == 0 and Wo % 2 == 0:              # upsample2 to (Ho, Wo) from (Ho / 2, Wo / 2)
                    i["xs"] = _rnd(torch.randn(N, Ho // 2, Wo // 2, C, generator=gen), dtype)
                yield f"N={N} Ho={Ho} Wo={Wo} C={C}", i


def _resample_ref(i, ft):
    r = dict(pool=_nhwc(O.resample(_nchw(i["x"].to(ft)), "down")) * (4.0 * i["scale"]))
    if i["xs"] is not None:
        r["up"] = _nhwc(O.resample(_nchw(i["xs"].to(ft)), "up")) * i["scale"]
    return r


def _resample_scl(i):
    r = dict(pool=_nhwc(O.resample(_nchw(i["x"].double().abs()), "down")) * (4.0 * abs(i["scale"])))
    if i["xs"] is not None:
        r["up"] = _nhwc(O.resample(_nchw(i["xs"].double().abs()), "up")) * abs(i["scale"])
    return r


def _resample_run(call, i, dtype, mis):
    N, Ho, Wo, C = i["N"], i["Ho"], i["Wo"], i["C"]
    pool = _buf((N, Ho, Wo, C), dtype, "out" in mis)
    call("hdmoe_pool2", pool, _dev(i["x"], dtype, "x" in mis), N, Ho, Wo, C, i["scale"], _dt(dtype))
    r = dict(pool=pool)
    if i["xs"] is not None:
        r["up"] = _buf((N, Ho, Wo, C), dtype, "out" in mis)
        call("hdmoe_upsample2", r["up"], _dev(i["xs"], dtype, "x" in mis), N, Ho, Wo, C, i["scale"], _dt(dtype))
    return r


_fam("resample2", dict(pool="pointwise", up="pointwise"), _resample_cases, _resample_ref, _resample_scl, _resample_run, ptrs=("out", "x"),
     mis_case=lambda dt: next(c for c in _resample_cases(dt) if c[0] == f"N=3 Ho=2 Wo=6 C={3 * _W(dt)}"))

FIR_TAPS = [[1.0, 1.0], [1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 5.0, 7.0, 7.0, 5.0, 3.0, 1.0]]


def _fir_geom(H, Wd, L):
    pad = (L - 1) // 2
    return pad, ((H + 2 * pad - L) // 2 + 1, (Wd + 2 * pad - L) // 2 + 1), ((H - 1) * 2 - 2 * pad + L, (Wd - 1) * 2 - 2 * pad + L)


def _fir_cases(dtype):
    for taps in FIR_TAPS:
        for H, Wd in ((2, 2), (5, 7), (8, 6)):
            for C in (1, 8):
                L = len(taps)
                pad, (Hd, Wdn), (Hu, Wu) = _fir_geom(H, Wd, L)
                gen = _gen(4500 + 10 * L + H + C)
                r = lambda *s: _rnd(torch.randn(*s, generator=gen), dtype)          # noqa: E731
                f = [_f32(t / sum(taps)) for t in taps]
                yield f"L={L} H={H} W={Wd} C={C}", dict(x=r(2, H, Wd, C), g=r(2, Hd, Wdn, C), taps=f, L=L, pad=pad, H=H, W=Wd, C=C,
                                                         dn=(Hd, Wdn), up=(Hu, Wu))


def _fir_ops(i, x, g, ft):
    """down(x), its adjoint applied to g (the backward of `down`, scale 1), and the forward `up` of x (scale 4), all NHWC, in ft."""
    C = i["C"]
    f = torch.tensor(i["taps"], dtype=torch.float64)
    k = torch.outer(f, f)[None, None].to(ft).repeat(C, 1, 1, 1)
    xc, gc = _nchw(x.to(ft)), _nchw(g.to(ft))
    down = F.conv2d(xc, k, stride=2, groups=C, padding=i["pad"])
    op = (i["H"] - ((i["dn"][0] - 1) * 2 - 2 * i["pad"] + i["L"]), i["W"] - ((i["dn"][1] - 1) * 2 - 2 * i["pad"] + i["L"]))
    adj = F.conv_transpose2d(gc, k, stride=2, groups=C, padding=i["pad"], output_padding=op)
    up = F.conv_transpose2d(xc, k * 4.0, stride=2, groups=C, padding=i["pad"])
    return dict(down=_nhwc(down), adj=_nhwc(adj), up=_nhwc(up))


def _fir_run(call, i, dtype, mis):
    N, H, Wd, C, L, pad = 2, i["H"], i["W"], i["C"], i["L"], i["pad"]
    x, g = _dev(i["x"], dtype), _dev(i["g"], dtype)
    down, adj, up = _buf((N, *i["dn"], C), dtype), _buf((N, H, Wd, C), dtype), _buf((N, *i["up"], C), dtype)
    call("hdmoe_fir_resample", down, x, i["taps"], L, pad, 1.0, 0, N, H, Wd, i["dn"][0], i["dn"][1], C, _dt(dtype))
    call("hdmoe_fir_resample", adj, g, i["taps"], L, pad, 1.0, 1, N, i["dn"][0], i["dn"][1], H, Wd, C, _dt(dtype))
    call("hdmoe_fir_resample", up, x, i["taps"], L, pad, 4.0, 1, N, H, Wd, i["up"][0], i["up"][1], C, _dt(dtype))
    return dict(down=down, adj=adj, up=up)


_fam("fir_resample", dict(down="reduction", adj="reduction", up="reduction"), _fir_cases, lambda i, ft: _fir_ops(i, i["x"], i["g"], ft),
     lambda i: _fir_ops(i, i["x"].abs(), i["g"].abs(), torch.float64), _fir_run)


# =====================================================================================================
# 5. row broadcast and reduce
# =====================================================================================================
def _seqred_cases(dtype):
    W = _W(dtype)
    table = [(W, (1, 3, 257)), (2 * W, (1, 3, 129)), (16 * W, (1, 3, 15, 17, 66)), (256 * W, (1, 3, 2, 6)), (3 * W, (1, 3, 7, 9, 34)),
             (5, (1, 3, 7, 9, 34))]
    for C, Ss in table:
        for S in Ss:
            for N in (1, 3):
                gen = _gen(5000 + C + 3 * S + N)
                yield f"C={C} S={S} N={N}", dict(x=_rnd(torch.randn(N, S, C, generator=gen) + 0.2, dtype), out0=torch.randn(N, C, generator=gen),
                                                 scale=_f32(0.37), N=N, S=S, C=C)


def _seqred_run(call, i, dtype, mis):
    out = _buf((i["N"], i["C"]), F32, fill=i["out0"])
    call("hdmoe_seq_reduce", out, _dev(i["x"], dtype, "x" in mis), i["N"], i["S"], i["C"], i["scale"], _dt(dtype))
    return dict(out=out)


_fam("seq_reduce", dict(out="reduction"), _seqred_cases, lambda i, ft: dict(out=i["out0"].to(ft) + i["scale"] * i["x"].to(ft).sum(1)),
     lambda i: dict(out=i["out0"].double().abs() + abs(i["scale"]) * i["x"].double().abs().sum(1)), _seqred_run, ptrs=("x",),
     mis_case=lambda dt: next(c for c in _seqred_cases(dt) if c[0] == f"C={16 * _W(dt)} S=17 N=3"))


def _bcast_cases(dtype):
    for N, S, C in ((1, 1, 1), (3, 5, 7), (2, 9, 16), (3, (CAP + 259) // 9, 3)):
        for has_x in (True, False):
            gen = _gen(5100 + N + S + C)
            yield f"N={N} S={S} C={C} x={'given' if has_x else 'null'}", dict(
                x=_rnd(torch.randn(N, S, C, generator=gen), dtype) if has_x else None, t=torch.randn(N, C, generator=gen), scale=_f32(-1.3),
                N=N, S=S, C=C)


def _bcast_ref(i, ft):
    v = (i["scale"] * i["t"].to(ft))[:, None, :].expand(i["N"], i["S"], i["C"])
    return dict(out=v.clone() if i["x"] is None else i["x"].to(ft) + v)


def _bcast_scl(i):
    v = (abs(i["scale"]) * i["t"].double().abs())[:, None, :].expand(i["N"], i["S"], i["C"])
    return dict(out=v if i["x"] is None else i["x"].double().abs() + v)


def _bcast_run(call, i, dtype, mis):
    out = _buf((i["N"], i["S"], i["C"]), dtype)
    call("hdmoe_seq_bcast_add", out, _dev(i["x"], dtype), _dev(i["t"], F32), i["N"], i["S"], i["C"], i["scale"], _dt(dtype))
    return dict(out=out)


_fam("seq_bcast_add", dict(out="pointwise"), _bcast_cases, _bcast_ref, _bcast_scl, _bcast_run)


def _srows_cases(dtype):
    W = _W(dtype)
    for L in (W, 8192, 8192 + W, 8193, 2048 * W + W):
        for rows in (1, 3):
            gen = _gen(5200 + L + rows)
            r = lambda: _rnd(torch.randn(rows, L, generator=gen) + 0.1, dtype)     # noqa: E731
            yield f"L={L} rows={rows}", dict(x=r(), dy=r(), s=torch.randn(rows, generator=gen) + 1.5, ds0=torch.randn(rows, generator=gen),
                                             rows=rows, L=L)
    for rows, L in ((3, (CAP + 259) // 3), (1, (CAP + 3) * W)):
        gen = _gen(5300 + rows)
        yield f"grid cap L={L} rows={rows}", dict(x=_rnd(torch.randn(rows, L, generator=gen), dtype), dy=None, s=torch.randn(rows, generator=gen),
                                                  ds0=None, rows=rows, L=L)


def _srows_ref(i, ft):
    x, s = i["x"].to(ft), i["s"].to(ft)
    r = dict(out=x * s[:, None])
    if i["dy"] is not None:
        dy = i["dy"].to(ft)
        dx, ds = dy * s[:, None], i["ds0"].to(ft) + (dy * x).sum(1)
        r.update(dx=dx, ds=ds, dx_only=dx, ds_only=ds)
    return r


def _srows_scl(i):
    r = dict(out=(i["x"].double() * i["s"].double()[:, None]).abs())
    if i["dy"] is not None:
        dx = (i["dy"].double() * i["s"].double()[:, None]).abs()
        ds = i["ds0"].double().abs() + (i["dy"].double() * i["x"].double()).abs().sum(1)
        r.update(dx=dx, ds=ds, dx_only=dx, ds_only=ds)
    return r


def _srows_run(call, i, dtype, mis):
    rows, L = i["rows"], i["L"]
    x, s = _dev(i["x"], dtype, "x" in mis), _dev(i["s"], F32)
    out = _buf((rows, L), dtype, "out" in mis)
    call("hdmoe_scale_rows_fwd", out, x, s, rows, L, _dt(dtype))
    r = dict(out=out)
    if i["dy"] is not None:
        dy = _dev(i["dy"], dtype, "dy" in mis)
        r.update(dx=_buf((rows, L), dtype, "dx" in mis), ds=_buf((rows,), F32, fill=i["ds0"]), dx_only=_buf((rows, L), dtype, "dx" in mis),
                 ds_only=_buf((rows,), F32, fill=i["ds0"]))
        call("hdmoe_scale_rows_bwd", r["dx"], r["ds"], dy, x, s, rows, L, _dt(dtype))
        call("hdmoe_scale_rows_bwd", r["dx_only"], None, dy, x, s, rows, L, _dt(dtype))
        call("hdmoe_scale_rows_bwd", None, r["ds_only"], dy, x, s, rows, L, _dt(dtype))
    return r


_fam("scale_rows", dict(out="pointwise", dx="pointwise", ds="reduction", dx_only="pointwise", ds_only="reduction"), _srows_cases, _srows_ref,
     _srows_scl, _srows_run, ptrs=("out", "x", "dx", "dy"),
     mis_case=lambda dt: next(c for c in _srows_cases(dt) if c[0] == f"L={8192 + _W(dt)} rows=3"))


def _bias_cases(dtype):
    for rows in (1, 63, 64, 65, 130):
        for L in (1, 255, 257):
            gen = _gen(5400 + rows + L)
            yield f"rows={rows} L={L}", dict(x=_rnd(torch.randn(rows, L, generator=gen) + 0.2, dtype), bias=torch.randn(L, generator=gen),
                                             out0=torch.randn(L, generator=gen), rows=rows, L=L)


def _bias_run(call, i, dtype, mis):
    x = _dev(i["x"], dtype)
    out, cs = _buf(x.shape, dtype), _buf((i["L"],), F32, fill=i["out0"])
    call("hdmoe_bias_add", out, x, _dev(i["bias"], F32), i["rows"], i["L"], _dt(dtype))
    call("hdmoe_colsum", cs, x, i["rows"], i["L"], _dt(dtype))
    return dict(out=out, colsum=cs)


_fam("bias_colsum", dict(out="pointwise", colsum="reduction"), _bias_cases,
     lambda i, ft: dict(out=i["x"].to(ft) + i["bias"].to(ft), colsum=i["out0"].to(ft) + i["x"].to(ft).sum(0)),
     lambda i: dict(out=i["x"].double().abs() + i["bias"].double().abs(), colsum=i["out0"].double().abs() + i["x"].double().abs().sum(0)),
     _bias_run)


def _film_cases(dtype):
    W = _W(dtype)
    for C in (W, 8 * W, 256 * W, 3 * W, 5):
        for HW in (1, 255, 256, 257):
            for N in (1, 3):
                gen = _gen(5500 + C + HW + N)
                u = _rnd(torch.randn(N, HW, C, generator=gen) * 1.5, dtype)
                k = min(C, len(SPECIALS))
                u[0, 0, :k] = _rnd(torch.tensor(SPECIALS[:k]), dtype)
                yield f"C={C} HW={HW} N={N}", dict(u=u, e=1.0 + 0.3 * torch.randn(N, C, generator=gen), de0=torch.randn(N, C, generator=gen),
                                                   da=_rnd(torch.randn(N, HW, C, generator=gen) + 0.25, dtype), N=N, HW=HW, C=C)


def _film_ref(i, ft):
    """out = mp_silu(u e); du = da mp_silu'(u e) e; de += sum over pixels of da mp_silu'(u e) u"""
    u, e = (i[k].to(ft).clone().requires_grad_(True) for k in ("u", "e"))
    out = O.mp_silu(u * e[:, None, :])
    du, de = torch.autograd.grad(out, (u, e), i["da"].to(ft))
    return dict(out=out.detach(), du=du, de=i["de0"].to(ft) + de)


def _film_scl(i):
    u, e, da = i["u"].double(), i["e"].double()[:, None, :], i["da"].double().abs()
    f, g, uf, ug = _silu_sc(u * e)
    return dict(out=(f, uf), du=(da * g * e.abs(), da * ug * e.abs()),
                de=(i["de0"].double().abs() + (da * g * u.abs()).sum(1), (da * ug * u.abs()).sum(1)))


def _film_run(call, i, dtype, mis):
    N, HW, C = i["N"], i["HW"], i["C"]
    u, e, da = _dev(i["u"], dtype, "u" in mis), _dev(i["e"], F32), _dev(i["da"], dtype, "da" in mis)
    out, du, de = _buf(u.shape, dtype, "out" in mis), _buf(u.shape, dtype, "du" in mis), _buf((N, C), F32, fill=i["de0"])
    call("hdmoe_film_silu_fwd", out, u, e, N, HW, C, _dt(dtype))
    call("hdmoe_film_silu_bwd", du, de, da, u, e, N, HW, C, _dt(dtype))
    return dict(out=out, du=du, de=de)


_fam("film_silu", dict(out="activation", du="activation", de="reduction"), _film_cases, _film_ref, _film_scl, _film_run,
     ptrs=("out", "u", "du", "da"), mis_case=lambda dt: next(c for c in _film_cases(dt) if c[0] == f"C={8 * _W(dt)} HW=257 N=3"))


def _lerp_cases(dtype):
    W = _W(dtype)
    for n in (W, 1000 * W, 262144 * W + W, 1001):
        for al in (0.0, 0.3, 1.0):
            gen = _gen(5600 + n % 9973)
            r = lambda: _rnd(torch.randn(n, generator=gen), dtype)                 # noqa: E731
            yield f"n={n} alpha={al}", dict(a=r(), b=r(), g=r(), alpha=_f32(al), d0=_f32(0.75))


def _lerp_ref(i, ft):
    a, b, g, al = i["a"].to(ft), i["b"].to(ft), i["g"].to(ft), i["alpha"]
    return dict(out=a + al * (b - a), da=(1.0 - al) * g, db=al * g, dalpha=(i["d0"] + (g * (b - a)).sum()).reshape(1))


def _lerp_scl(i):
    a, b, g, al = i["a"].double().abs(), i["b"].double().abs(), i["g"].double().abs(), abs(i["alpha"])
    return dict(out=a + al * (a + b), da=abs(1.0 - al) * g, db=al * g, dalpha=(abs(i["d0"]) + (g * (a + b)).sum()).reshape(1))


def _lerp_run(call, i, dtype, mis):
    a, b, g = _dev(i["a"], dtype, "a" in mis), _dev(i["b"], dtype, "b" in mis), _dev(i["g"], dtype, "g" in mis)
    alpha = torch.tensor([i["alpha"]], dtype=F32, device=DEV)
    out, da, db = _buf(a.shape, dtype), _buf(a.shape, dtype, "da" in mis), _buf(a.shape, dtype, "db" in mis)
    dalpha = _buf((1,), F32, fill=torch.tensor([i["d0"]]))
    call("hdmoe_lerp_param_fwd", out, a, b, alpha, a.numel(), _dt(dtype))
    call("hdmoe_lerp_param_bwd", da, db, dalpha, g, a, b, alpha, a.numel(), _dt(dtype))
    return dict(out=out, da=da, db=db, dalpha=dalpha)


_fam("lerp_param", dict(out="pointwise", da="pointwise", db="pointwise", dalpha="reduction"), _lerp_cases, _lerp_ref, _lerp_scl, _lerp_run,
     ptrs=("da", "db", "g", "a", "b"), mis_case=lambda dt: next(c for c in _lerp_cases(dt) if c[0] == f"n={1000 * _W(dt)} alpha=0.3"))


# =====================================================================================================
# 6. gate, softmax and the fp32 vector-path ops
# =====================================================================================================
GAPS = [0.0, 30.0, -30.0, 100.0, -100.0, 1.5, -0.25]


def _gate_inputs(C, rows, dtype, seed, first_gap=0):
    gen = _gen(seed)
    r = lambda *s: _rnd(torch.randn(*s, generator=gen), dtype)                     # noqa: E731
    l0 = r(rows)
    gaps = torch.tensor([GAPS[(first_gap + j) % len(GAPS)] for j in range(rows)])
    lg = torch.stack([l0, _rnd(l0 + gaps, dtype)], 1)
    gate = torch.softmax(lg.double(), 1).float()             # the backward's input: the stored fp32 gate
    return dict(lg=lg, U=r(rows, C), A=r(rows, C), dout=r(rows, C), dgate=torch.randn(rows, 2, generator=gen), gate=gate, rows=rows, C=C)


def _gate_cases(dtype):
    W = _W(dtype)
    j = 0
    for C in (W, 2 * W, 16 * W, 64 * W, 3 * W, 65 * W, 128 * W, 5):
        for rows in (1, 3, 33):
            j += 1
            yield f"C={C} rows={rows}", _gate_inputs(C, rows, dtype, 6000 + C + rows, first_gap=j)
    yield "grid cap, scalar", _gate_inputs(9, (CAP + 259) // 9, dtype, 6001)
    yield "grid cap, vec", _gate_inputs(W, CAP + 3, dtype, 6002)


def _gate_ref(i, ft):
    """g = softmax(logits); out = k (U + g0 U + g1 A), k = 0.5 / sqrt(0.5).  Backward from the stored gate: go = k dout, dU = go (1 + g0),
    dA = go g1, d_j = dgate_j + sum_c go (U | A), dlogits_j = g_j (d_j - (d0 g0 + d1 g1)); once with dgate and once without."""
    g = torch.softmax(i["lg"].to(ft), 1)
    U_, A_ = i["U"].to(ft), i["A"].to(ft)
    r = dict(gate=g, out=GATE_K * (U_ + g[:, :1] * U_ + g[:, 1:] * A_))
    gs = i["gate"].to(ft)
    go = GATE_K * i["dout"].to(ft)
    r.update(dU=go * (1.0 + gs[:, :1]), dA=go * gs[:, 1:])
    for key, dg in (("dlogits", i["dgate"].to(ft)), ("dlogits_nodgate", 0.0)):
        d = torch.stack([(go * U_).sum(1), (go * A_).sum(1)], 1) + dg
        r[key] = gs * (d - (d * gs).sum(1, keepdim=True))
    return r


def _gate_scl(i):
    lg = i["lg"].double()
    g = torch.softmax(lg, 1)
    sg = g * (1.0 + (1.0 - g) * (lg[:, :1] - lg[:, 1:]).abs())
    U_, A_ = i["U"].double().abs(), i["A"].double().abs()
    r = dict(gate=(sg, TINY), out=(GATE_K * (U_ + sg[:, :1] * U_ + sg[:, 1:] * A_), TINY * GATE_K * (U_ + A_)))
    gs = i["gate"].double()
    go = GATE_K * i["dout"].double().abs()
    r.update(dU=go * (1.0 + gs[:, :1]), dA=(go * gs[:, 1:], TINY * go))
    for key, dg in (("dlogits", i["dgate"].double().abs()), ("dlogits_nodgate", 0.0)):
        D = torch.stack([(go * U_).sum(1), (go * A_).sum(1)], 1) + dg
        r[key] = (gs * (D + (D * gs).sum(1, keepdim=True)), TINY * D.sum(1, keepdim=True).expand_as(gs))
    return r


def _gate_run(call, i, dtype, mis):
    rows, C = i["rows"], i["C"]
    lg, U_, A_ = _dev(i["lg"], dtype), _dev(i["U"], dtype, "U" in mis), _dev(i["A"], dtype, "A" in mis)
    dout, gs = _dev(i["dout"], dtype, "dout" in mis), _dev(i["gate"], F32)
    r = dict(gate=_buf((rows, 2), F32), out=_buf((rows, C), dtype, "out" in mis), dU=_buf((rows, C), dtype, "dU" in mis),
             dA=_buf((rows, C), dtype, "dA" in mis), dlogits=_buf((rows, 2), dtype), dlogits_nodgate=_buf((rows, 2), dtype))
    call("hdmoe_gate_mix_fwd", r["out"], r["gate"], lg, U_, A_, rows, C, _dt(dtype))
    call("hdmoe_gate_mix_bwd", r["dU"], r["dA"], r["dlogits"], dout, _dev(i["dgate"], F32), gs, U_, A_, rows, C, _dt(dtype))
    dU2, dA2 = _buf((rows, C), dtype, "dU" in mis), _buf((rows, C), dtype, "dA" in mis)
    call("hdmoe_gate_mix_bwd", dU2, dA2, r["dlogits_nodgate"], dout, None, gs, U_, A_, rows, C, _dt(dtype))
    torch.cuda.synchronize()
    assert torch.equal(dU2, r["dU"]) and torch.equal(dA2, r["dA"]), "gate_mix_bwd: dU / dA depend on dgate"
    return r


_fam("gate_mix", dict(gate="softmax", out="softmax", dU="pointwise", dA="pointwise", dlogits="softmax", dlogits_nodgate="softmax"),
     _gate_cases, _gate_ref, _gate_scl, _gate_run, ptrs=("out", "U", "A", "dU", "dA", "dout"),
     mis_case=lambda dt: ("C=16W rows=33", _gate_inputs(16 * _W(dt), 33, dt, 6003)),
     zeros=dict(dlogits=False, dlogits_nodgate=False))     # g = 1: d - (d g0 + d1 g1) cancels


def _softmax_cases(dtype):
    for C in (1, 2, 3, 8):
        for rows in (1, 257, CAP + 259):
            if rows > CAP and C != 2:
                continue
            for scale in (1.0, 2.5):
                gen = _gen(6100 + C + rows)
                spread = torch.tensor([1.0, 10.0, 100.0])[torch.arange(rows) % 3][:, None]
                x = torch.randn(rows, C, generator=gen) * spread
                if C > 1:
                    x[0::4, -1] = x[0::4, 0] - 100.0
                    x[1::4, -1] = x[1::4, 0] + 100.0
                y = (scale * torch.softmax(x.double(), 1)).float()                 # the backward's input: the stored forward result
                yield f"C={C} rows={rows} scale={scale}", dict(x=x, y=y, dy=torch.randn(rows, C, generator=gen), scale=_f32(scale), rows=rows, C=C)
                if rows > CAP:
                    break


def _softmax_ref(i, ft):
    """y = scale softmax(x); dx = y (dy - sum(dy y) / scale)"""
    y, dy = i["y"].to(ft), i["dy"].to(ft)
    return dict(out=i["scale"] * torch.softmax(i["x"].to(ft), 1), dx=y * (dy - (dy * y).sum(1, keepdim=True) / i["scale"]))


def _softmax_scl(i):
    x = i["x"].double()
    p, d = torch.softmax(x, 1), (x - x.amax(1, keepdim=True)).abs()
    y, dy, sc = i["y"].double().abs(), i["dy"].double().abs(), abs(i["scale"])
    return dict(out=(sc * p * (1.0 + d + (p * d).sum(1, keepdim=True)), TINY * sc),
                dx=(y * (dy + (dy * y).sum(1, keepdim=True) / sc), TINY * (dy + (dy * y).sum(1, keepdim=True) / sc)))


def _softmax_run(call, i, dtype, mis):
    out, dx = _buf((i["rows"], i["C"]), F32), _buf((i["rows"], i["C"]), F32)
    call("hdmoe_softmax_rows_fwd", out, _dev(i["x"], F32), i["rows"], i["C"], i["scale"])
    call("hdmoe_softmax_rows_bwd", dx, _dev(i["dy"], F32), _dev(i["y"], F32), i["rows"], i["C"], i["scale"])
    return dict(out=out, dx=dx)


_fam("softmax_rows", dict(out="softmax", dx="softmax"), _softmax_cases, _softmax_ref, _softmax_scl, _softmax_run, dtypes=(F32,),
     zeros=dict(dx=False))                                 # C = 1: dy - dy y / scale cancels


def _adaln_cases(dtype):
    for B in (1, 5):
        for Fd in (1, 3, 64):
            gen = _gen(6200 + B + Fd)
            yield f"B={B} F={Fd}", dict(x=torch.randn(B, Fd, generator=gen), cond=torch.randn(B, 2 * Fd, generator=gen),
                                        g=torch.randn(B, Fd, generator=gen), B=B, F=Fd)


def _adaln_ref(i, ft):
    """out = x (1 + gamma) + beta, cond = [gamma | beta]; dx = g (1 + gamma), dcond = [g x | g]"""
    x, c, g, Fd = i["x"].to(ft), i["cond"].to(ft), i["g"].to(ft), i["F"]
    return dict(out=x * (1.0 + c[:, :Fd]) + c[:, Fd:], dx=g * (1.0 + c[:, :Fd]), dcond=torch.cat([g * x, g], 1))


def _adaln_scl(i):
    x, c, g, Fd = i["x"].double().abs(), i["cond"].double().abs(), i["g"].double().abs(), i["F"]
    return dict(out=x * (1.0 + c[:, :Fd]) + c[:, Fd:], dx=g * (1.0 + c[:, :Fd]), dcond=torch.cat([g * x, g], 1))


def _adaln_run(call, i, dtype, mis):
    B, Fd = i["B"], i["F"]
    x, c = _dev(i["x"], F32), _dev(i["cond"], F32)
    out, dx, dcond = _buf((B, Fd), F32), _buf((B, Fd), F32), _buf((B, 2 * Fd), F32)
    call("hdmoe_adaln_fwd", out, x, c, B, Fd)
    call("hdmoe_adaln_bwd", dx, dcond, _dev(i["g"], F32), x, c, B, Fd)
    return dict(out=out, dx=dx, dcond=dcond)


_fam("adaln", dict(out="pointwise", dx="pointwise", dcond="pointwise"), _adaln_cases, _adaln_ref, _adaln_scl, _adaln_run, dtypes=(F32,))


def _embed_cases(dtype):
    for B in (1, 7):
        gen = _gen(6300 + B)
        sigma = torch.exp(torch.rand(B, generator=gen) * 10.6 - 6.2)               # 0.002 .. 80
        sigma[0] = 1.0                                       # c_noise = log(1) / 4 = 0 exactly
        yield f"B={B}", dict(x=torch.randn(B, generator=gen) * 1.5, freqs=torch.randn(32, generator=gen) * 6.0,
                             phases=torch.rand(32, generator=gen) * 6.2831853, sigma=sigma, sd=_f32(0.5), B=B,
                             cn=torch.randn(B, generator=gen), tp=_f32(0.3), soft=_f32(0.7))


def _embed_ref(i, ft):
    """fourier: oracle.mp_fourier's formula, sqrt(2) cos(x (x) freqs + phases); edm_coeffs: c_skip = sd^2 / (s^2 + sd^2), c_out = s sd /
    sqrt(s^2 + sd^2), c_in = 1 / sqrt(s^2 + sd^2), c_noise = log(s) / 4 (oracle.preconditioned_hdmoem), with one sigma for all B and with
    one each; sigmoid_scaling: w = sigmoid((4 c - tp) / soft), s_vit = 2 (w + 0.01), s_unet = 2 ((1 - w) + 0.01)."""
    x, fr, ph, s, sd, B = i["x"].to(ft), i["freqs"].to(ft), i["phases"].to(ft), i["sigma"].to(ft), i["sd"], i["B"]
    r = dict(fourier=(torch.outer(x, fr) + ph).cos() * math.sqrt(2.0))
    for key, sg in (("coef", s), ("coef1", s[:1].expand(B))):
        q = sg * sg + sd * sd
        r[key] = torch.stack([sd * sd / q, sg * sd / q.sqrt(), 1.0 / q.sqrt(), sg.log() / 4.0])
    w = torch.sigmoid((i["cn"].to(ft) * 4.0 - i["tp"]) / i["soft"])
    c001 = _f32(1e-2)
    r.update(sv=(w + c001) * 2.0, su=((1.0 - w) + c001) * 2.0)
    r["pair"] = torch.stack([r["sv"], r["su"]], 1)
    return r


def _embed_scl(i):
    r = {k: v.abs() for k, v in _embed_ref(i, torch.float64).items()}
    x, fr, ph = i["x"].double().abs(), i["freqs"].double().abs(), i["phases"].double().abs()
    r["fourier"] = math.sqrt(2.0) * (1.0 + torch.outer(x, fr) + ph)                # |d cos| <= the rounding of its argument
    zs = (i["cn"].double().abs() * 4.0 + abs(i["tp"])) / abs(i["soft"])           # 4 c - tp may cancel
    w = torch.sigmoid((i["cn"].double() * 4.0 - i["tp"]) / i["soft"])
    sw = 2.0 * (1.0 + w * (1.0 - w) * zs)
    r.update(sv=r["sv"] + sw, su=r["su"] + sw, pair=r["pair"] + sw[:, None])
    return r


def _embed_run(call, i, dtype, mis):
    B, Fd = i["B"], i["freqs"].numel()
    r = dict(fourier=_buf((B, Fd), F32), coef=_buf((4, B), F32), coef1=_buf((4, B), F32), sv=_buf((B,), F32), su=_buf((B,), F32),
             pair=_buf((B, 2), F32))
    sigma = _dev(i["sigma"], F32)
    call("hdmoe_fourier", r["fourier"], _dev(i["x"], F32), _dev(i["freqs"], F32), _dev(i["phases"], F32), B, Fd)
    call("hdmoe_edm_coeffs", r["coef"], sigma, B, i["sd"], B)
    call("hdmoe_edm_coeffs", r["coef1"], sigma, 1, i["sd"], B)
    call("hdmoe_sigmoid_scaling", r["sv"], r["su"], r["pair"], _dev(i["cn"], F32), i["tp"], i["soft"], B)
    return r


_fam("embeddings", dict(fourier="pointwise", coef="pointwise", coef1="pointwise", sv="activation", su="activation", pair="activation"),
     _embed_cases, _embed_ref, _embed_scl, _embed_run, dtypes=(F32,))


def _layout_cases(dtype):
    for C in (1, 3, 4):
        for HW in (1, 35):
            gen = _gen(6400 + C + HW)
            yield f"C={C} HW={HW}", dict(x=torch.randn(2, C, HW, generator=gen), s=torch.randn(2, generator=gen) + 1.5, C=C, HW=HW)


def _layout_run(call, i, dtype, mis):
    out = _buf((2, i["HW"], i["C"]), dtype)
    call("hdmoe_nchw_to_nhwc", out, _dev(i["x"], F32), _dev(i["s"], F32), 2, i["C"], i["HW"], _dt(dtype))
    return dict(out=out)


_fam("nchw_to_nhwc", dict(out="pointwise"), _layout_cases,
     lambda i, ft: dict(out=(i["x"].to(ft) * i["s"].to(ft)[:, None, None]).permute(0, 2, 1).contiguous()),
     lambda i: dict(out=(i["x"].double() * i["s"].double()[:, None, None]).abs().permute(0, 2, 1).contiguous()), _layout_run)


def _sumn_cases(dtype):
    W = _W(dtype)
    for n in (1, 2, 16):
        for nelem in (W, 3 * W + 1, 1024 + W, 1024 + 2 * W - 1):
            for scaled in (False, True):
                gen = _gen(6500 + n + nelem)
                yield f"n={n} nelem={nelem} src_scale={'given' if scaled else 'null'}", dict(
                    srcs=[_rnd(torch.randn(nelem, generator=gen), dtype) for _ in range(n)],
                    sc=[_f32(v) for v in (torch.randn(n, generator=gen) + 0.5)] if scaled else None)


def _sumn_ref(i, ft):
    """out = sum_k src_scale[k] srcs[k], in the kernel's order (k ascending)"""
    sc = i["sc"] or [1.0] * len(i["srcs"])
    out = sc[0] * i["srcs"][0].to(ft)
    for k in range(1, len(sc)):
        out = out + sc[k] * i["srcs"][k].to(ft)
    return dict(out=out)


def _sumn_raw(out, srcs, sc, n, nelem, dtype):
    """hdmoe_sum_n through ctypes: the binding's `call` cannot pass a null src_scale."""
    import ctypes
    import hdmoe_hip
    from hdmoe_hip._lib import _ptr_array
    arr = _ptr_array(srcs)
    fs = None if sc is None else (ctypes.c_float * len(sc))(*sc)
    return hdmoe_hip.lib().hdmoe_sum_n(out.data_ptr(), ctypes.cast(arr, ctypes.c_void_p), None if fs is None else ctypes.cast(fs, ctypes.c_void_p),
                                       n, nelem, _dt(dtype), torch.cuda.current_stream().cuda_stream)


def _sumn_run(call, i, dtype, mis):
    srcs = [_dev(s, dtype) for s in i["srcs"]]
    out = _buf(srcs[0].shape, dtype)
    assert _sumn_raw(out, srcs, i["sc"], len(srcs), srcs[0].numel(), dtype) == 0
    return dict(out=out)


_fam("sum_n", dict(out="reduction"), _sumn_cases, _sumn_ref,
     lambda i: dict(out=sum(abs(c) * s.double().abs() for c, s in zip(i["sc"] or [1.0] * len(i["srcs"]), i["srcs"]))), _sumn_run)


# =====================================================================================================
# the tests
# =====================================================================================================
def _fam_params():
    return [pytest.param(n, dt, id=f"{n}-{'fp32' if dt == F32 else 'bf16'}") for n, f in FAMS.items() for dt in f.dtypes]


@gpu
@pytest.mark.parametrize("name,dtype", _fam_params())
def test_against_fp64(lib, name, dtype):
    """Every case table, every output, against the float64 reference under the class bound."""
    _run_family(lib, name, dtype)


@gpu
@pytest.mark.parametrize("name,dtype", [p for p in _fam_params() if FAMS[p.values[0]].ptrs])
def test_misaligned_pointer_takes_scalar_arm(lib, name, dtype):
    """A view one element into a larger buffer, for each pointer the host code tests with al16 in turn, at a shape that otherwise takes the
    vector arm: the scalar arm gives the same truth."""
    _run_misaligned(lib, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_cat2_silu_fwd(lib, dtype):
    """out against oracle.mp_cat; out_h against float64 mp_silu of the kernel's own stored `out`."""
    fam = FAMS["cat2"]
    for tag, i in _cat_silu_cases(dtype):
        if i["gcat"] is None:
            continue
        a = _rnd(i["xcat"][:, :i["Ca"]], dtype)              # inputs that carry the special activation points
        b = _rnd(i["xcat"][:, i["Ca"]:], dtype)
        i = dict(i, a=a, b=b)
        out, out_h = _buf(i["dout"].shape, dtype), _buf(i["dout"].shape, dtype)
        lib("hdmoe_cat2_silu_fwd", out, out_h, _dev(a, dtype), _dev(b, dtype), i["wa"], i["wb"], i["Ca"], i["Cb"], i["rows"], _dt(dtype))
        torch.cuda.synchronize()
        _guards_ok(tag)
        r = fam.ref(i, torch.float64)["out"]
        _match(out, r, _bound(r, r.abs(), K_PW, dtype), f"cat2_silu_fwd {tag}: out", cls="pointwise")
        z = out.detach().cpu().double()
        f, _, uf, _ = _silu_sc(z)
        h = O.mp_silu(z)
        _match(out_h, h, _bound(h, f, K_ACT, dtype, uf), f"cat2_silu_fwd {tag}: out_h", cls="activation")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_entries_without_scalar_arm_decline(lib, dtype):
    """hdmoe_sum_n, hdmoe_mp_silu_bwd_add and hdmoe_cat2_silu_* have no scalar arm: a misaligned pointer or a count that is no multiple of
    W is declined before any launch, and a pre-filled output stays as it was."""
    W, d = _W(dtype), _dt(dtype)
    n = 4 * W
    t = lambda m=False: _dev(torch.ones(n), dtype, m)                              # noqa: E731
    o = lambda m=False: _buf((n,), dtype, m, fill=7.0)                             # noqa: E731
    # mp_silu_bwd_add: dx, dy, x, gx
    for k in range(4):
        a = [o(k == 0), t(k == 1), t(k == 2), t(k == 3)]
        _raises_and_keeps(lib, "hdmoe_mp_silu_bwd_add", a[0], a[0], a[1], a[2], a[3], 0.7, n, d)
    out = o()
    _raises_and_keeps(lib, "hdmoe_mp_silu_bwd_add", out, out, t(), t(), t(), 0.7, n - 1, d)
    # cat2_silu_fwd: out, out_h, a, b at (Ca, Cb) = (W, 3W), one row; cat2_silu_bwd: da, db, gcat, gh, xcat
    for k in range(4):
        a = [o(k == 0), o(k == 1), _dev(torch.ones(1, W), dtype, k == 2), _dev(torch.ones(1, 3 * W), dtype, k == 3)]
        _raises_and_keeps(lib, "hdmoe_cat2_silu_fwd", a[k] if k < 2 else a[0], a[0], a[1], a[2], a[3], 0.5, 0.5, W, 3 * W, 1, d)
    for k in range(5):
        a = [_buf((W,), dtype, k == 0, fill=7.0), _buf((3 * W,), dtype, k == 1, fill=7.0), t(k == 2), t(k == 3), t(k == 4)]
        _raises_and_keeps(lib, "hdmoe_cat2_silu_bwd", a[1] if k == 1 else a[0], a[0], a[1], a[2], a[3], a[4], 0.5, 0.5, W, 3 * W, 1, d)
    for Ca, Cb in ((3, 5), (W, W + 1)):
        out, out_h = _buf((Ca + Cb,), dtype, fill=7.0), _buf((Ca + Cb,), dtype, fill=7.0)
        a, b, g = _dev(torch.ones(1, Ca), dtype), _dev(torch.ones(1, Cb), dtype), _dev(torch.ones(1, Ca + Cb), dtype)
        _raises_and_keeps(lib, "hdmoe_cat2_silu_fwd", out, out, out_h, a, b, 0.5, 0.5, Ca, Cb, 1, d)
        da, db = _buf((Ca,), dtype, fill=7.0), _buf((Cb,), dtype, fill=7.0)
        _raises_and_keeps(lib, "hdmoe_cat2_silu_bwd", da, da, db, g, g, g, 0.5, 0.5, Ca, Cb, 1, d)
    # sum_n: out or one source misaligned; 17 sources
    for k in range(3):
        out, srcs = o(k == 0), [t(k == 1), t(k == 2)]
        before = out.clone()
        assert _sumn_raw(out, srcs, None, 2, n, dtype) == -1
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    out = o()
    assert _sumn_raw(out, [t() for _ in range(17)], None, 17, n, dtype) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _GUARDS.clear()


@gpu
def test_declines_before_launch(lib):
    """The remaining declines of the entries tested here, each a status the host code returns before any launch."""
    f = lambda *s: torch.ones(*s, device=DEV)                                      # noqa: E731
    out = torch.full((64,), 7.0, device=DEV)
    x = f(64)
    _raises_and_keeps(lib, "hdmoe_upsample2", out, out, x, 1, 1, 1, 4, 1.0, 0)                       # odd Ho and Wo
    _raises_and_keeps(lib, "hdmoe_upsample2", out, out, x, 1, 5, 4, 1, 1.0, 0)                       # odd Ho
    _raises_and_keeps(lib, "hdmoe_fir_resample", out, out, x, [1.0 / 9] * 9, 9, 4, 1.0, 0, 1, 8, 8, 4, 4, 1, 0)   # L = 9
    assert lib("hdmoe_fir_resample", out, x, [0.5, 0.5], 2, 0, 1.0, 0, 0, 4, 4, 2, 2, 1, 0) == 0     # N = 0: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    big = f(8196)
    o2 = torch.full((8196,), 7.0, device=DEV)
    _raises_and_keeps(lib, "hdmoe_seq_reduce", o2, o2, big, 1, 1, 8196, 1.0, 0)                      # C > 8192
    _raises_and_keeps(lib, "hdmoe_scale_rows_bwd", out, out, None, x, x, x, 65536, 4, 0)             # rows > 65535
    _raises_and_keeps(lib, "hdmoe_film_silu_bwd", out, out, out.clone(), x, x, x, 65536, 1, 4, 0)    # N > 65535
    _raises_and_keeps(lib, "hdmoe_edm_coeffs", out, out, x, 2, 0.5, 7)                               # nsig = 2, B = 7
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        lib("hdmoe_cast", out, x, 8, 3, 1)                                                           # f16 -> bf16
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        lib("hdmoe_cast", out, x, 8, 1, 3)                                                           # bf16 -> f16
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@gpu
def test_cast_is_exact(lib):
    """hdmoe_cast, all six dtype pairs, bit for bit against Tensor.to: ties to even, NaN, overflow to +-inf, signed zeros."""
    from hdmoe_hip._lib import dtype_code_cast
    gen = _gen(7000)
    sp = torch.tensor([0.0, -0.0, NAN, float("inf"), -float("inf"), 3.4e38, -3.4e38, 3.3895e38, 65504.0, 65519.0, 65520.0, -65520.0, 70000.0, 1e30,
                       1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -12,
                       -1.0 - 2.0 ** -8, 2049.0, 2051.0])
    x32 = torch.cat([sp, torch.randn(1024 + 7, generator=gen) * 100.0])
    for din, dout in ((F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (torch.float16, F32), (F32, torch.float16)):
        x = x32.to(din).to(DEV)
        out = torch.zeros(x.numel(), dtype=dout, device=DEV)
        lib("hdmoe_cast", out, x, x.numel(), dtype_code_cast(din), dtype_code_cast(dout))
        want = x.cpu().to(dout)
        got = out.cpu()
        nan = want.isnan()
        assert torch.equal(got.isnan(), nan), (din, dout)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (din, dout, int((_bits(got)[~nan] != _bits(want)[~nan]).sum()))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ops(lib, dtype):
    """upsample2 with scale 1 and nchw_to_nhwc without a scale move values: bit for bit.  seq_reduce twice on the same input: the same
    bits (its comment promises a fixed summation order).  known_blend keeps x where the mask is 0, bit for bit."""
    W, d = _W(dtype), _dt(dtype)
    gen = _gen(7100)
    for C in (W, 3 * W, 3):
        xs = _rnd(torch.randn(3, 1, 3, C, generator=gen), dtype)
        out = _buf((3, 2, 6, C), dtype)
        lib("hdmoe_upsample2", out, _dev(xs, dtype), 3, 2, 6, C, 1.0, d)
        assert torch.equal(out.cpu().float(), xs.repeat_interleave(2, 1).repeat_interleave(2, 2)), f"upsample2 C={C}"
    for tag, i in _layout_cases(dtype):
        out = _buf((2, i["HW"], i["C"]), dtype)
        lib("hdmoe_nchw_to_nhwc", out, _dev(i["x"], F32), None, 2, i["C"], i["HW"], d)
        assert torch.equal(out.cpu(), i["x"].permute(0, 2, 1).contiguous().to(dtype)), f"nchw_to_nhwc {tag}"
    for tag, i in _seqred_cases(dtype):
        a, b = (_seqred_run(lib, i, dtype, ())["out"] for _ in range(2))
        assert torch.equal(a, b), f"seq_reduce {tag}: two calls differ"
    for tag, i in _blend_cases(dtype):
        got = _blend_run(lib, i, dtype, ())["x"].cpu().float()
        assert torch.equal(got[i["m"] == 0], i["x"][i["m"] == 0]), f"known_blend {tag}: x changed where the mask is 0"
    torch.cuda.synchronize()
    _guards_ok("exact ops")


@gpu
def test_take_col_pos(lib):
    """out[b] = w[b][e] where > 0, else 0 (NaN -> 0); the backward writes g[b] only where w[b][e] > 0 and leaves the rest of dw alone."""
    gen = _gen(7200)
    for E in (1, 4):
        for B in (1, 9):
            w = torch.randn(B, E, generator=gen)
            w.view(-1)[0::3] = 0.0
            w.view(-1)[1::4] = NAN
            w.view(-1)[2::5] = -0.0
            g = torch.randn(B, generator=gen)
            wd, gd = w.to(DEV), g.to(DEV)
            for e in range(E):
                out, dw = _buf((B,), F32), _buf((B, E), F32, fill=7.0)
                lib("hdmoe_take_col_pos_fwd", out, wd, B, E, e)
                lib("hdmoe_take_col_pos_bwd", dw, gd, wd, B, E, e)
                pos = w[:, e] > 0
                assert torch.equal(out.cpu(), torch.where(pos, w[:, e], torch.zeros(B))), (E, B, e)
                want = torch.full((B, E), 7.0)
                want[:, e] = torch.where(pos, g, want[:, e])
                assert torch.equal(dw.cpu(), want), (E, B, e)
    _guards_ok("take_col_pos")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_fir_adjoint(lib, dtype):
    """<down(x), g> = <x, up(g)> from the kernel outputs, in float64, within the bound of a sum (each side rounds its outputs once more
    in bf16)."""
    fam = FAMS["fir_resample"]
    for tag, i in _fir_cases(dtype):
        got = _fir_run(lib, i, dtype, ())
        x, g = i["x"].double(), i["g"].double()
        lhs, rhs = (got["down"].cpu().double() * g).sum(), (x * got["adj"].cpu().double()).sum()
        sc = fam.scl(i)
        terms = (sc["down"] * g.abs()).sum() + (x.abs() * sc["adj"]).sum()
        bound = (K_RED * U + (2.0 ** -8 if dtype == BF16 else 0.0)) * terms
        assert abs(float(lhs - rhs)) <= float(bound), f"fir adjoint {tag}: {float(lhs)} vs {float(rhs)}, bound {float(bound):.3e}"
    _GUARDS.clear()


# =====================================================================================================
# CPU only: the matcher bites
# =====================================================================================================
def _stored(r, dtype=F32):
    """r as a kernel stores it"""
    return r.to(dtype)


def test_match_rejects_injected_faults():
    """_match with the class bounds, applied to the float64 references of the case tables: the correct result, rounded as the kernels
    store it, passes; each way a subtly wrong kernel would differ is rejected.  Needs no GPU."""
    def ok(fam, i, key, k, dtype=F32):
        ref, sc = fam.ref(i, torch.float64), fam.scl(i)
        scale, under = _split(sc[key])
        _match(k, ref[key].double(), _bound(ref[key].double(), scale, KS[fam.cls[key]], dtype, under), f"{fam.name}: {key}")

    def rejected(*a, **kw):
        with pytest.raises(AssertionError):
            ok(*a, **kw)

    for dtype in (F32, BF16):
        W = _W(dtype)
        # the last partial vector dropped (left as the buffer's fill, or as zeros): axpby at n = 257
        fam = FAMS["axpby"]
        i = next(c for t, c in fam.cases(dtype) if t.startswith("n=257 "))
        r = fam.ref(i, torch.float64)["out"]
        ok(fam, i, "out", _stored(r, dtype), dtype)
        bad = r.clone(); bad[-(257 % W):] = NAN
        rejected(fam, i, "out", _stored(bad, dtype), dtype)
        bad = r.clone(); bad[-(257 % W):] = 0.0
        rejected(fam, i, "out", _stored(bad, dtype), dtype)
        # wa / wb swapped
        fam = FAMS["cat2"]
        i = next(c for t, c in fam.cases(dtype) if t == f"Ca={W} Cb={W} rows=7")
        r = fam.ref(i, torch.float64)
        ok(fam, i, "out", _stored(r["out"], dtype), dtype)
        bad = torch.cat([i["a"].double() * i["wb"], i["b"].double() * i["wa"]], 1)
        rejected(fam, i, "out", _stored(bad, dtype), dtype)
        # one pixel-row offset in pool2
        fam = FAMS["resample2"]
        i = next(c for t, c in fam.cases(dtype) if t == f"N=3 Ho=5 Wo=4 C={W}")
        r = fam.ref(i, torch.float64)["pool"]
        ok(fam, i, "pool", _stored(r, dtype), dtype)
        shifted = fam.ref(dict(i, x=torch.roll(i["x"], -1, 1)), torch.float64)["pool"]
        rejected(fam, i, "pool", _stored(shifted, dtype), dtype)
        # one chunk missing from a row sum: scale_rows_bwd's ds without its second chunk (one vector / one element long)
        fam = FAMS["scale_rows"]
        for L, first in ((2048 * W + W, 2048 * W), (8193, 8192)):
            i = next(c for t, c in fam.cases(dtype) if t == f"L={L} rows=3")
            r = fam.ref(i, torch.float64)["ds"]
            ok(fam, i, "ds", _stored(r))
            part = i["ds0"].double() + (i["dy"].double() * i["x"].double())[:, :first].sum(1)
            rejected(fam, i, "ds", _stored(part))
            # a += replaced by =
            rejected(fam, i, "ds", _stored(r - i["ds0"].double()))
        fam = FAMS["seq_reduce"]
        i = next(c for t, c in fam.cases(dtype) if t == f"C={16 * W} S=66 N=3")
        r = fam.ref(i, torch.float64)["out"]
        ok(fam, i, "out", _stored(r))
        rejected(fam, i, "out", _stored(r - i["scale"] * i["x"].double()[:, 64:].sum(1)))     # the rows of the last pass of the R = 16 lanes
        rejected(fam, i, "out", _stored(r - i["out0"].double()))
        # a gate row taken from its neighbour
        fam = FAMS["gate_mix"]
        i = next(c for t, c in fam.cases(dtype) if t == f"C={2 * W} rows=33")
        r = fam.ref(i, torch.float64)
        ok(fam, i, "out", _stored(r["out"], dtype), dtype)
        g = torch.roll(r["gate"], 1, 0)
        U_, A_ = i["U"].double(), i["A"].double()
        rejected(fam, i, "out", _stored(GATE_K * (U_ + g[:, :1] * U_ + g[:, 1:] * A_), dtype), dtype)
        rejected(fam, i, "gate", _stored(g))


# =====================================================================================================
# calibration (CPU): `PYTHONPATH=. python tests/test_elementwise_kernels.py`
# =====================================================================================================
def _calibrate():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    worst = {}
    for name, fam in FAMS.items():
        for dtype in fam.dtypes:
            for tag, i in fam.cases(dtype):
                r64, r32, sc = fam.ref(i, torch.float64), fam.ref(i, F32), fam.scl(i)
                for key, r in r64.items():
                    scale, under = _split(sc[key])
                    r, k = r.double(), r32[key].double()
                    assert torch.equal(k.isnan(), r.isnan()) and torch.equal(k.isinf(), r.isinf()), (name, tag, key)
                    b = (U * (r.abs() + scale) + under + TINY).expand_as(r)
                    assert bool((k[(b == 0)] == r[(b == 0)]).all()), (name, tag, key)
                    ratio = float(((k - r).abs() / b.clamp_min(1e-300)).max()) if r.numel() else 0.0
                    c = fam.cls[key]
                    if ratio > worst.get(c, (0.0,))[0]:
                        worst[c] = (ratio, f"{name} {tag} {key} {str(dtype).replace('torch.', '')}")
    for c, (ratio, where) in sorted(worst.items()):
        K = 2.0 ** math.ceil(math.log2(4.0 * ratio))
        print(f"{c:11s} worst fp32-CPU ratio {ratio:6.2f} ({where})   4 x worst {4 * ratio:6.2f}   K {K:g}   (the file has {KS[c]:g})")


if __name__ == "__main__":
    _calibrate()
