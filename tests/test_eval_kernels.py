"""The held-out evaluation kernels at their edges (csrc/evalstats.hip: hdmoe_eval_inputs, hdmoe_eval_accumulate through ops.eval_inputs /
ops.eval_accumulate): items, levels and sigmas exactly, the target bit for bit, the noise against ops.randn_keyed per (item, level) key
and -- the property the evaluation rests on -- independent of batch size, position and round; the statistics table against numpy fp64
on the same fp32 inputs, its determinism, NaN containment, accumulation, and every argument error before anything is written."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234ABCD5678EF01
SENTINEL = -7.0
PAD = 64
U = 2.0 ** -24                                                # unit roundoff of fp32


def _padded(shape, dtype, sentinel=SENTINEL):
    """A tensor of `shape` at the front of a sentinel-filled flat buffer that is PAD elements longer: (view, flat)."""
    n = int(np.prod(shape))
    flat = torch.full((n + PAD,), sentinel, dtype=dtype, device=DEV)
    return flat[:n].view(shape), flat


def _tail_untouched(view, flat, sentinel=SENTINEL):
    return bool((flat[view.numel():] == sentinel).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _mean(N, chw, dtype):
    """The dataset's table, made once per shape and storage type and never written."""
    g = torch.Generator(device=DEV).manual_seed(3)
    return (0.5 * torch.randn((N,) + chw, device=DEV, generator=g)).to(dtype)


def _levels(K):
    return torch.exp(torch.linspace(-3.0, 3.0, K, dtype=torch.float64)).to(torch.float32).to(DEV) if K > 1 \
        else torch.tensor([0.75], dtype=torch.float32, device=DEV)


def _follows(out, base, mult, eps_ref):
    """out = base + mult eps_ref in the tolerance form of test_latent_dataset.py's noise check: the recovered draw within
    1e-5 max(|eps_ref|, 1) / min(|mult|, 1), or -- where mult eps_ref is below the last bits of base -- out within 1e-6 of the sum."""
    out, base, mult = out.double(), base.double(), mult.double()
    eps = (out - base) / mult
    tol = 1e-5 * eps_ref.abs().clamp(min=1.0) / mult.abs().clamp(max=1.0)
    ok = (eps - eps_ref).abs() <= tol
    ref = base + mult * eps_ref
    under = (mult * eps_ref).abs() < 2.0 ** -20 * base.abs()
    ok |= under & ((out - ref).abs() <= 1e-6 * ref.abs())
    return bool(ok.all()), float(((eps - eps_ref).abs() / tol).max())


def _run_inputs(mean, B, levels, rnd, first, count, *, scale=1.0, offset=0, seed=SEED):
    """ops.eval_inputs into sentinel-padded buffers; offset = 1 shifts x and x0 by one float (no 16-byte alignment: the scalar path)."""
    from hdmoe_hip import ops
    chw = tuple(mean.shape[1:])
    n = B * int(np.prod(chw))
    v, f = {}, {}
    for k in ("x", "x0"):
        f[k] = torch.full((n + PAD + offset,), SENTINEL, dtype=torch.float32, device=DEV)[offset:]
        v[k] = f[k][:n].view((B,) + chw)
    v["sigma"], f["sigma"] = _padded((B, 1, 1, 1), torch.float32)
    v["level"], f["level"] = _padded((B,), torch.int32, -7)
    v["item"], f["item"] = _padded((B,), torch.int32, -7)
    ops.eval_inputs(v["x"], v["x0"], v["sigma"], v["level"], v["item"], mean, levels, seed, rnd, first, count, scale=scale)
    return v, f


@functools.lru_cache(maxsize=None)
def _eps_row(chw, key, seed=SEED):
    """The draw of one (item, level) key, through the library's own keyed generator: shared by every case that meets the key."""
    from hdmoe_hip import ops
    return ops.randn_keyed(torch.empty(chw, device=DEV), seed ^ ops.EVAL_SALT, key).double()


# (N, B, (C,H,W)): one row per batch with chw % 4 != 0; the 16-byte path; chw % 4 == 0 with W % 4 != 0 (still the 16-byte path: nothing is
# mirrored, a vector may straddle image rows); more than one workgroup of single vectors with B no multiple of anything.
SHAPES = [(5, 1, (3, 5, 7)), (10, 4, (4, 8, 8)), (7, 8, (4, 8, 6)), (300, 257, (1, 2, 2))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,B,chw", SHAPES, ids=[f"N{s[0]}-B{s[1]}-{'x'.join(map(str, s[2]))}" for s in SHAPES])
def test_eval_inputs_follow_the_contract(N, B, chw, dtype):
    mean = _mean(N, chw, dtype)
    worst = 0.0
    for K in (1, 3, 64):
        levels = _levels(K)
        for rnd in sorted({0, K - 1}):
            first = N - 1 + (N if K == 3 else 0)              # the items wrap past N inside the batch (B > 1), from a start beyond N too
            count = max(B - 2, 0) if rnd == 0 else B          # count < B, count == 0 at B = 1, and the full batch
            scale = 0.09 if K == 3 else 1.0
            for offset in ((0, 1) if K == 3 else (0,)):
                v, f = _run_inputs(mean, B, levels, rnd, first, count, scale=scale, offset=offset)
                torch.cuda.synchronize()
                where = (K, rnd, first, count, offset)
                for k in v:
                    assert _tail_untouched(v[k], f[k], -7 if v[k].dtype == torch.int32 else SENTINEL), (k, where)
                item = (first + np.arange(B)) % N
                lvl = (item + rnd) % K
                assert np.array_equal(v["item"].cpu().numpy(), item), where
                assert np.array_equal(v["level"].cpu().numpy(), np.where(np.arange(B) < count, lvl, -1)), where
                assert torch.equal(v["sigma"].view(-1), levels[torch.from_numpy(lvl).to(DEV)]), where        # padding rows too: finite
                want = mean[torch.from_numpy(item).to(DEV)].float() * float(np.float32(scale))             # one fp32 product per element
                assert torch.equal(_bits(v["x0"]), _bits(want)), where
                eps = torch.stack([_eps_row(chw, int(it) * K + int(k)) for it, k in zip(item, lvl)])
                ok, r = _follows(v["x"], v["x0"], v["sigma"].expand_as(v["x"]), eps)
                worst = max(worst, r)
                assert ok, where
                # x = fma(sigma, eps, x0) bit for bit from the library's own draw (gen_noise_kernel's expression)
                e32 = eps.float()
                fma = torch.addcmul(v["x0"].double(), v["sigma"].double().expand_as(e32), e32.double()).float()      # exact product, one rounding
                assert torch.equal(_bits(v["x"]), _bits(fma)), where
    print(f"max |draw - ref| / tol = {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_noise_of_an_item_level_pair_is_independent_of_batch_position_and_round(dtype):
    """The x row of (item, level) made at B = 1, at B = 8 in another position and in another round is bit-identical: the number an
    evaluation reports belongs to the weights alone."""
    N, chw, K = 7, (4, 8, 6), 3
    mean, levels = _mean(N, chw, dtype), _levels(K)
    item, lvl = 5, 1
    rnd1 = (lvl - item) % K                                   # (item + round) % K == lvl
    a, _ = _run_inputs(mean, 1, levels, rnd1, item, 1)
    assert int(a["item"][0]) == item and int(a["level"][0]) == lvl
    b, _ = _run_inputs(mean, 8, levels, rnd1, 3, 8)           # items 3 4 5 6 0 1 2 3: position 2
    assert int(b["item"][2]) == item and int(b["level"][2]) == lvl
    c, _ = _run_inputs(mean, 8, levels, rnd1 + K, N + 1, 6)   # another round with the same level map, start beyond N: position 4
    assert int(c["item"][4]) == item and int(c["level"][4]) == lvl
    d, _ = _run_inputs(mean, 5, levels, rnd1, item, 5, offset=1)          # the scalar path, position 0
    for other, pos in ((b, 2), (c, 4), (d, 0)):
        assert torch.equal(_bits(a["x"][0]), _bits(other["x"][pos])) and torch.equal(_bits(a["x0"][0]), _bits(other["x0"][pos]))
    e, _ = _run_inputs(mean, 8, levels, rnd1 + 1, 3, 8)       # the same item at another level: another draw
    assert int(e["item"][2]) == item and int(e["level"][2]) != lvl
    assert not torch.equal((a["x"][0] - a["x0"][0]) / a["sigma"][0], (e["x"][2] - e["x0"][2]) / e["sigma"][2])
    g, _ = _run_inputs(mean, 1, levels, rnd1, item, 1, seed=SEED + 1)     # another seed: another draw, the same target
    assert torch.equal(_bits(a["x0"]), _bits(g["x0"])) and not torch.equal(a["x"], g["x"])


# ------------------------------------------------------------------------------------------------------------------ the statistics
# Longest chain of fp32 additions behind one partial sum of squares (csrc/evalstats.hip eval_sse_kernel): a chunk of 4096 elements over
# 256 threads is 16 terms per thread, then 6 butterfly steps inside a wave, then the 4 wave sums one after the other: 16 + 6 + 4.
# Chunks and samples are summed in double.  Every term is non-negative, so |got - ref| <= 4 M U ref covers the M - 1 additions and the
# three roundings of a term ((d - t) once, its square once, counted twice in the product) with room to spare.
M_CHAIN = 16 + 6 + 4
SSE_TOL = 4 * M_CHAIN * U
SIGMA_DATA = 0.5


def _stat_inputs(B, L, E, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    d = torch.randn(B, L, device=DEV, generator=g)
    t = torch.randn(B, L, device=DEV, generator=g)
    sigma = torch.exp(torch.randn(B, device=DEV, generator=g)).view(B, 1, 1, 1)
    level = torch.randint(-1, K, (B,), device=DEV, generator=g, dtype=torch.int32)          # -1: padding rows among them
    lv = (6.0 * torch.randn(B, device=DEV, generator=g)).view(B, 1, 1, 1)                      # beyond the clamp at +-10 now and then
    pU = torch.rand(B, E, device=DEV, generator=g)
    pU = torch.where(torch.rand(B, E, device=DEV, generator=g) < 0.4, torch.zeros_like(pU), pU)     # top-k gates: exact zeros
    pV = torch.rand(B, E, device=DEV, generator=g)
    pV = torch.where(torch.rand(B, E, device=DEV, generator=g) < 0.4, torch.zeros_like(pV), pV)
    return d, t, sigma, level, lv, pU, pV


def _stat_ref(d, t, sigma, level, lv, pU, pV, K):
    """numpy fp64 on the same fp32 inputs: (table (K, 6 + 4E), the non-negative part of the nll column per level, sum |lv| per level)."""
    d, t = d.double().cpu().numpy(), t.double().cpu().numpy()
    B, E = pU.shape
    sg = sigma.double().cpu().numpy().reshape(B)
    lvl = level.cpu().numpy()
    l = np.zeros(B) if lv is None else np.clip(lv.double().cpu().numpy().reshape(B), -10.0, 10.0)
    pu, pv = pU.double().cpu().numpy(), pV.double().cpu().numpy()
    mse = ((d - t) ** 2).sum(1) / d.shape[1]
    w = (sg ** 2 + SIGMA_DATA ** 2) / (sg * SIGMA_DATA) ** 2
    acc = np.zeros((K, 6 + 4 * E))
    pos, absl = np.zeros(K), np.zeros(K)
    for k in range(K):
        m = lvl == k
        acc[k, :6] = [m.sum(), mse[m].sum(), (mse[m] ** 2).sum(), (w[m] * mse[m]).sum(), (mse[m] * np.exp(-l[m]) + l[m]).sum(), l[m].sum()]
        acc[k, 6:] = np.concatenate([pu[m].sum(0), (pu[m] > 0).sum(0), pv[m].sum(0), (pv[m] > 0).sum(0)])
        pos[k], absl[k] = (mse[m] * np.exp(-l[m])).sum(), np.abs(l[m]).sum()
    return acc, pos, absl


def _accumulate(acc, d, t, sigma, level, lv, pU, pV, ws=None):
    from hdmoe_hip import ops
    B, L = d.shape[0], d[0].numel()
    if ws is None:
        ws = torch.full((ops.eval_ws_floats(B, L),), SENTINEL, dtype=torch.float32, device=DEV)
    ops.eval_accumulate(acc, ws, d, t, sigma, level, lv, pU, pV, SIGMA_DATA)
    return ws


def _check_table(got, ref, pos, absl, E, where, times=1.0):
    """Counts and selection counts exact, sums of probabilities and of lv to 1e-12 relative, what comes from the sums of squares to
    SSE_TOL relative; the nll column mixes the two: SSE_TOL of its non-negative part plus 1e-12 of sum |lv| (lv has either sign)."""
    sel = np.r_[0, 6 + E + np.arange(E), 6 + 3 * E + np.arange(E)]
    assert np.array_equal(got[:, sel], times * ref[:, sel]), where
    prob = np.r_[6 + np.arange(E), 6 + 2 * E + np.arange(E)]
    assert np.all(np.abs(got[:, prob] - times * ref[:, prob]) <= 1e-12 * times * ref[:, prob]), where
    assert np.all(np.abs(got[:, 5] - times * ref[:, 5]) <= 1e-12 * times * absl), where
    err = np.abs(got[:, 1:4] - times * ref[:, 1:4]) / np.maximum(times * ref[:, 1:4], 1e-300)
    assert np.all(err <= np.array([SSE_TOL, 2 * SSE_TOL, SSE_TOL])), (where, err.max(0))           # mse^2: the relative error of a square
    assert np.all(np.abs(got[:, 4] - times * ref[:, 4]) <= times * (SSE_TOL * pos + 1e-12 * absl)), where
    return float(err.max())


@pytest.mark.parametrize("L", [105, 256, 4097], ids=lambda v: f"L{v}")                             # 4097: one element above the chunk size
@pytest.mark.parametrize("B", [1, 5, 257], ids=lambda v: f"B{v}")
def test_eval_accumulate_against_fp64(B, L):
    from hdmoe_hip import ops
    assert ops.eval_chunk() == 4096 and ops.eval_ws_floats(B, L) == B * (2 if L == 4097 else 1)
    worst = 0.0
    for n, (E, K) in enumerate([(1, 1), (4, 3), (8, 64), (4, 64), (8, 3)]):
        d, t, sigma, level, lv, pU, pV = _stat_inputs(B, L, E, K, seed=n)
        if n == 1:
            level = torch.full_like(level, K - 1)                                                  # all rows in one level, the others empty
        if n == 4:
            level = torch.where(level == 1, torch.full_like(level, -1), level)                     # an empty level among used ones
        for with_lv in (True, False):
            lvv = lv if with_lv else None
            ref, pos, absl = _stat_ref(d, t, sigma, level, lvv, pU, pV, K)
            acc, flat = _padded((K, 6 + 4 * E), torch.float64)
            acc.zero_()
            _accumulate(acc, d, t, sigma, level, lvv, pU, pV)
            one = acc.clone()
            where = (E, K, with_lv)
            worst = max(worst, _check_table(one.cpu().numpy(), ref, pos, absl, E, where))
            assert _tail_untouched(acc, flat), where
            _accumulate(acc, d, t, sigma, level, lvv, pU, pV)                                      # += : two calls in a row
            _check_table(acc.cpu().numpy(), ref, pos, absl, E, where, times=2.0)
            again = torch.zeros_like(one)
            _accumulate(again, d, t, sigma, level, lvv, pU, pV)
            assert torch.equal(one.view(torch.int64), again.view(torch.int64)), where              # the same inputs: the same bits
    print(f"B={B} L={L}: worst relative error of an SSE-derived sum {worst:.3e} (bound {SSE_TOL:.3e}, M = {M_CHAIN})")


def test_eval_accumulate_largest_batch_and_table():
    """B = 4096 rows (16 tiles of the finish kernel), K E at their limits (2432 sums over 256 threads), levels beyond K skipped."""
    B, L, E, K = 4096, 105, 8, 64
    d, t, sigma, level, lv, pU, pV = _stat_inputs(B, L, E, K)
    level = level.clone()
    level[7], level[4000] = K, 2 ** 30                                                             # never produced by eval_inputs: skipped
    ref, pos, absl = _stat_ref(d, t, sigma, level, lv, pU, pV, K)
    acc, flat = _padded((K, 6 + 4 * E), torch.float64)
    acc.zero_()
    _accumulate(acc, d, t, sigma, level, lv, pU, pV)
    _check_table(acc.cpu().numpy(), ref, pos, absl, E, "B4096")
    assert _tail_untouched(acc, flat) and ref[:, 0].sum() < B - 2


def test_nan_reaches_its_own_level_only():
    B, L, E, K = 257, 256, 4, 3
    d, t, sigma, level, lv, pU, pV = _stat_inputs(B, L, E, K)
    ref, pos, absl = _stat_ref(d, t, sigma, level, lv, pU, pV, K)
    b = int((level == 1).nonzero()[0])
    d = d.clone()
    d[b, 17] = float("nan")
    acc = torch.zeros(K, 6 + 4 * E, dtype=torch.float64, device=DEV)
    _accumulate(acc, d, t, sigma, level, lv, pU, pV)
    got = acc.cpu().numpy()
    assert np.isnan(got[1, 1:5]).all() and not np.isnan(np.delete(got, 1, 0)).any() and not np.isnan(got[1, [0, 5]]).any()
    keep = np.isfinite(got)
    fixed = np.where(keep, got, ref)
    _check_table(fixed, ref, pos, absl, E, "nan")                                                  # everything else is what it was
    # a NaN gate probability: its level's sum of that column, not its selection count, nothing else
    pU2 = pU.clone()
    pU2[b, 2] = float("nan")
    acc.zero_()
    _accumulate(acc, t + (d - t).nan_to_num(0.0), t, sigma, level, lv, pU2, pV)
    got = acc.cpu().numpy()
    assert np.isnan(got[1, 6 + 2]) and np.isnan(got).sum() == 1


# ------------------------------------------------------------------------------------------------------------------ errors
def test_errors_raise_before_anything_is_written():
    """Every HDMOE_EINVAL / HDMOE_EDTYPE case of both entry points, through the raw binding (the wrappers' own checks come first and are
    exercised below): an error status and untouched sentinel buffers."""
    from hdmoe_hip import _lib
    N, B, chw, K, E, L = 6, 4, 48, 3, 4, 48
    mean = torch.randn(N, chw, device=DEV)
    levels = _levels(K)
    out = {k: torch.full((B * chw + 8,), SENTINEL, device=DEV) for k in ("x", "x0")}
    out["sigma"] = torch.full((B + 8,), SENTINEL, device=DEV)
    out["level"] = torch.full((B + 8,), -7, dtype=torch.int32, device=DEV)
    out["item"] = torch.full((B + 8,), -7, dtype=torch.int32, device=DEV)
    good = dict(x=out["x"], x0=out["x0"], sigma=out["sigma"], level=out["level"], item=out["item"], mean=mean, dtype=_lib.F32, levels=levels,
                seed=SEED, round=0, first=0, count=B, B=B, chw=chw, N=N, K=K, scale=1.0)
    bad = [dict(x=None), dict(x0=None), dict(sigma=None), dict(level=None), dict(item=None), dict(mean=None), dict(levels=None),
           dict(x0=out["x"]), dict(B=0), dict(chw=0), dict(N=0), dict(K=0), dict(K=65), dict(B=4097), dict(count=-1), dict(count=B + 1),
           dict(first=-1), dict(round=-1), dict(scale=float("nan")), dict(dtype=2), dict(dtype=_lib.F16)]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(RuntimeError, match="unsupported dtype" if "dtype" in kw else "invalid argument"):
            _lib.call("hdmoe_eval_inputs", *a.values())
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t == (-7 if t.dtype == torch.int32 else SENTINEL)).all()), k

    d, t, sigma, level, lv, pU, pV = _stat_inputs(B, L, E, K)
    acc = torch.full((K * (6 + 4 * E) + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.full((B + 8,), SENTINEL, device=DEV)
    good = dict(acc=acc, ws=ws, d=d, t=t, sigma=sigma, level=level, lv=lv, pU=pU, pV=pV, B=B, L=L, E=E, K=K, sd=SIGMA_DATA)
    bad = [dict(acc=None), dict(ws=None), dict(d=None), dict(t=None), dict(sigma=None), dict(level=None), dict(pU=None), dict(pV=None),
           dict(B=0), dict(B=4097), dict(L=0), dict(E=0), dict(E=9), dict(K=0), dict(K=65)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid argument"):
            _lib.call("hdmoe_eval_accumulate", *dict(good, **kw).values())
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all()) and bool((ws == SENTINEL).all())


def test_wrappers_raise_value_error_before_anything_is_written():
    from hdmoe_hip import ops
    N, B, chw, K, E = 6, 4, (3, 4, 4), 3, 4
    mean, levels = _mean(N, chw, torch.float32), _levels(K)
    v, f = _run_inputs(mean, B, levels, 0, 0, B)
    for k in v:
        v[k].fill_(-7 if v[k].dtype == torch.int32 else SENTINEL)
    call = lambda **kw: ops.eval_inputs(**dict(dict(x=v["x"], x0=v["x0"], sigma=v["sigma"], level=v["level"], item=v["item"], mean=mean,
                                                    levels=levels, seed=SEED, round=0, first=0, count=B), **kw))
    for kw in (dict(x=v["x"][:, :, :, :2]), dict(x=v["x"].double()), dict(x=v["x0"]), dict(level=v["level"].float()), dict(item=v["item"][:2]),
               dict(mean=mean.double()), dict(mean=mean[:, :2]), dict(levels=levels.view(1, K)), dict(levels=levels.double()),
               dict(levels=torch.ones(65, device=DEV)), dict(count=B + 1), dict(count=-1), dict(first=-1), dict(round=-1),
               dict(scale=float("nan")), dict(sigma=v["sigma"][:2])):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError):
        call(mean=mean.cpu())
    torch.cuda.synchronize()
    for k in v:
        assert bool((v[k] == (-7 if v[k].dtype == torch.int32 else SENTINEL)).all()), k
    d, t, sigma, level, lv, pU, pV = _stat_inputs(B, 48, E, K)
    acc = torch.full((K, 6 + 4 * E), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.full((B,), SENTINEL, device=DEV)
    call = lambda **kw: ops.eval_accumulate(**dict(dict(acc=acc, ws=ws, denoised=d, x0=t, sigma=sigma, level=level, log_var=lv, pU=pU, pV=pV,
                                                        sigma_data=SIGMA_DATA), **kw))
    for kw in (dict(acc=acc.float()), dict(acc=acc[:, :-1]), dict(ws=ws[:B - 1]), dict(ws=ws.double()), dict(denoised=d.double()),
               dict(x0=t[:, :40]), dict(level=level.long()), dict(pV=pV[:, :2]), dict(pU=pU.t()), dict(log_var=lv[:2]),
               dict(sigma=sigma[:2]), dict(pU=torch.zeros(B, 9, device=DEV), pV=torch.zeros(B, 9, device=DEV),
                                           acc=torch.zeros(K, 42, dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError):
        call(denoised=d.cpu(), x0=t.cpu())
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all()) and bool((ws == SENTINEL).all())
