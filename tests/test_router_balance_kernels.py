"""hdmoe_router_head_bias_fwd and hdmoe_balance_bias_update (csrc/router.hip) against inline fp64 / integer numpy references.

The head with a selection bias picks its top-k over xout + bias and weighs the picked experts by the softmax of the RAW xout; the update
moves the bias by a fixed rate towards the under-loaded experts.  What is compared, and with which bound:

  * zero bias: every output bit for bit the plain head's (hdmoe_router_head_fwd), all-masked rows included (NaN bits too).
  * random bias: the picked SET equals the fp64 top-k of xout + bias (ties to the lowest index).  The kernel adds xout + bias in fp32 (one
    rounding, <= 2^-24 * 8 ~ 5e-7 at these magnitudes), so rows whose k-th and (k+1)-th biased scores are closer than 1e-4 are left out; the
    inputs (unit-normal logits, |bias| <= 2) keep those rows under 5 % on the reference alone, which `test_reference_inputs_...` checks on
    the CPU.  The ORDER inside idx is checked against the kernel's own arithmetic: fp32 scores (numpy's fp32 add is the same correctly
    rounded add) never increase along idx, and equal scores come in index order.
  * gate weights: w_j = exp(d_j) / sum_i exp(d_i), d = xout - max over the picked.  fp32 error model: d carries one rounding (|d| 2^-24
    absolute, the same relative error in exp), expf <= 2 ulp (2^-22), the k-term sum <= k 2^-24, the division 2^-24; numerator and
    denominator together: relative <= (2 (dmax + 4) + k + 1) 2^-24, plus one fp32 denormal step (2e-38) where the kernel may flush.
  * backward: hdmoe_router_head_bwd from the saved idx; fp64 gradient with idx held constant.  Bound: 4 (E + 40) 2^-24 times the sum of the
    cotangents' maxima (each of the three terms is a product with a probability <= 1 computed to (40 + E) 2^-24, and an E-term dot).
  * accumulators and the update: integers and dyadic floats -- exact.
  * convergence: the device loop against an fp64 simulation of the same loop on the same inputs.
"""
import functools

import numpy as np
import pytest
import torch

DEV = torch.device("cuda:0")
gpu = pytest.mark.gpu
U = 2.0 ** -24
SHIFT = 20
EK = [(1, 1), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 8), (64, 1), (64, 2), (64, 64)]
BS = (1, 63, 257)


# ------------------------------------------------------------------------------------------------------------------ inputs and references
def _inputs(B, E, k, noisy, masked, seed):
    """float32 numpy (logits, noise, mask, bias).  Masked cases hold, where B allows, an all-masked row (row 0), rows with fewer allowed
    experts than k (rows 1, 2: one allowed expert) and random rows."""
    rng = np.random.default_rng(1000 * seed + 17 * B + 3 * E + k)
    logits = rng.standard_normal((B, E)).astype(np.float32)
    noise = (0.3 * rng.standard_normal((B, E))).astype(np.float32) if noisy else None
    mask = None
    if masked:
        mask = (rng.random((B, E)) < 0.7).astype(np.float32)
        for b in range(B):
            if mask[b].sum() == 0:
                mask[b, rng.integers(E)] = 1.0
        if B > 1:
            mask[0] = 0.0
        for b in (1, 2):
            if B > b:
                mask[b] = 0.0
                mask[b, (5 * b) % E] = 1.0
    bias = rng.uniform(-2.0, 2.0, E).astype(np.float32)
    return logits, noise, mask, bias


def _xout(logits, noise, mask):
    x = logits if noise is None else logits + noise            # fp32 + fp32: the kernel's add
    if mask is not None:
        x = np.where(mask == 0, np.float32(-np.inf), x)
    return x.astype(np.float32)


def _ref_topk(x32, bias, k):
    """fp64: (idx (B, k) by descending biased score, ties to the lowest index; near-tie rows (B,) bool)."""
    score = x32.astype(np.float64) + bias.astype(np.float64)[None, :]
    order = np.argsort(-score, axis=1, kind="stable")
    idx = order[:, :k]
    near = np.zeros(len(score), dtype=bool)
    if k < score.shape[1]:
        rows = np.arange(len(score))
        a, b = score[rows, order[:, k - 1]], score[rows, order[:, k]]
        fin = np.isfinite(a) & np.isfinite(b)
        near[fin] = (a[fin] - b[fin]) < 1e-4
    return idx, near


def _ref_weights(x32, idx):
    """fp64 softmax of the raw xout over idx -> (sparse (B, E), dmax (B,)); all-masked rows NaN."""
    B, E = x32.shape
    x = x32.astype(np.float64)
    rows = np.arange(B)[:, None]
    sel = x[rows, idx]
    top = sel.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = sel - top
        w = np.exp(d)
        w = w / w.sum(1, keepdims=True)
    sparse = np.zeros((B, E))
    sparse[rows, idx] = w
    sparse[np.isnan(w).any(1)] = np.nan
    dfin = np.where(np.isfinite(d), np.abs(d), 0.0)
    return sparse, dfin.max(1)


def _t(a, dtype=torch.float32):
    return None if a is None else torch.tensor(a, dtype=dtype, device=DEV)


def _head(logits, noise, mask, k, bias=None, accum=None):
    from hdmoe_hip import ops
    out = ops.router_head(_t(logits), _t(noise), _t(mask), k, sel_bias=_t(bias), accum=accum)
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _shares(mask, B, E, k):
    """Python integers: (allowed (B, E) bool, share per row)."""
    allowed = np.ones((B, E), dtype=bool) if mask is None else mask != 0
    share = []
    for b in range(B):
        a = int(allowed[b].sum())
        share.append(0 if a == 0 else ((min(k, a) << (SHIFT + 1)) + a) // (2 * a))      # round(2^20 min(k, a) / a), never a tie for a <= 64
    return allowed, share


def _ref_counts(idx, mask, B, E, k):
    allowed, share = _shares(mask, B, E, k)
    load, target = [0] * E, [0] * E
    for b in range(B):
        for e in range(E):
            if allowed[b, e]:
                target[e] += share[b]
        for e in idx[b]:
            if allowed[b, int(e)]:
                load[int(e)] += 1
    return load, target


ALL_CASES = [(B, E, k, noisy, masked) for E, k in EK for B in BS for noisy, masked in ((False, False), (True, True), (False, True), (True, False))]


def test_reference_inputs_leave_out_at_most_five_percent_of_the_rows():
    """CPU: the near-tie rule applied to the reference alone, per case and overall."""
    rows = out = 0
    for B, E, k, noisy, masked in ALL_CASES:
        logits, noise, mask, bias = _inputs(B, E, k, noisy, masked, 1)
        _, near = _ref_topk(_xout(logits, noise, mask), bias, k)
        assert near.sum() <= 0.05 * B, (B, E, k, noisy, masked, int(near.sum()))
        rows, out = rows + B, out + int(near.sum())
    print(f"near-tie rows left out: {out} of {rows}")
    assert out <= 0.05 * rows


# ------------------------------------------------------------------------------------------------------------------ the head
@gpu
@pytest.mark.parametrize("E,k", EK)
def test_zero_bias_is_the_plain_head_bit_for_bit(E, k):
    for B in BS:
        for noisy, masked in ((False, False), (True, True)):
            logits, noise, mask, _ = _inputs(B, E, k, noisy, masked, 0)
            old = _head(logits, noise, mask, k)
            new = _head(logits, noise, mask, k, bias=np.zeros(E, np.float32))
            for name, a, b in zip(("sparse", "probs", "xout", "idx"), old, new):
                assert torch.equal(_bits(a), _bits(b)), (name, B, E, k, noisy, masked)
            if masked and B > 1:                                 # the all-masked row, as in the plain head: NaN probabilities, the lowest
                assert bool(torch.isnan(new[1][0]).all())        # k indices picked at NaN weight, 0 elsewhere
                assert new[3][0].tolist() == list(range(k)) and bool(torch.isnan(new[0][0, :k]).all()) and bool((new[0][0, k:] == 0).all())


@gpu
@pytest.mark.parametrize("E,k", EK)
def test_random_bias_against_fp64(E, k):
    worst = 0.0
    for B in BS:
        for noisy, masked in ((False, False), (True, True), (False, True), (True, False)):
            logits, noise, mask, bias = _inputs(B, E, k, noisy, masked, 1)
            x32 = _xout(logits, noise, mask)
            ridx, near = _ref_topk(x32, bias, k)
            assert near.sum() <= 0.05 * B
            sparse, probs, xout, idx = _head(logits, noise, mask, k, bias=bias)
            plain = _head(logits, noise, mask, k)
            assert torch.equal(_bits(probs), _bits(plain[1])) and torch.equal(_bits(xout), _bits(plain[2]))    # the bias reaches neither
            assert np.array_equal(xout.cpu().numpy().view(np.int32), x32.view(np.int32))
            got = idx.cpu().numpy().astype(np.int64)
            keep = ~near
            assert np.array_equal(np.sort(got[keep], 1), np.sort(ridx[keep], 1)), (B, E, k, noisy, masked)
            # the order inside idx, in the kernel's own fp32 arithmetic: scores never increase; equal scores in index order
            s32 = (x32 + bias[None, :]).astype(np.float32)
            sc = s32[np.arange(B)[:, None], got]
            assert bool((sc[:, :-1] >= sc[:, 1:]).all())
            assert bool((got[:, :-1] < got[:, 1:])[sc[:, :-1] == sc[:, 1:]].all())
            assert all(len(set(r)) == k for r in got.tolist())
            # gate weights: fp64 softmax of the raw xout over the picked set (the kernel's own set on the rows left out)
            ref, dmax = _ref_weights(x32, got)
            sp = sparse.cpu().numpy().astype(np.float64)
            nan_rows = np.isnan(ref).any(1)
            assert np.array_equal(np.isnan(sp).any(1), nan_rows) and (mask is None or np.array_equal(nan_rows, mask.sum(1) == 0))
            fin = ~nan_rows
            bound = (2.0 * (dmax[fin, None] + 4.0) + k + 1) * U * ref[fin] + 2e-38
            err = np.abs(sp[fin] - ref[fin])
            worst = max(worst, float((err / bound).max()) if fin.any() else 0.0)
            assert bool((err <= bound).all()), (B, E, k, noisy, masked, float((err / bound).max()))
            assert bool((sp[fin][ref[fin] == 0] == 0).all())     # off the picked set, and masked picks: exactly 0
    print(f"E={E} k={k}: worst gate-weight error / bound = {worst:.3f}")


@gpu
@pytest.mark.parametrize("E,k", [(8, 1), (8, 2), (8, 8), (64, 2), (64, 64)])
def test_exact_ties_go_to_the_lowest_index(E, k):
    """Quarter-valued logits and biases: the sums are exact in fp32 and fp64 alike, ties abound, and idx is compared in order."""
    rng = np.random.default_rng(5 + E + k)
    B = 63
    logits = (rng.integers(-4, 5, (B, E)) / 4.0).astype(np.float32)
    bias = (rng.integers(-4, 5, E) / 4.0).astype(np.float32)
    logits[0] = 1.0 - bias                                       # every biased score of row 0 equal: picks 0 .. k-1
    for mask in (None, (rng.random((B, E)) < 0.6).astype(np.float32)):
        x32 = _xout(logits, None, mask)
        ridx, _ = _ref_topk(x32, bias, k)
        score = x32.astype(np.float64) + bias[None, :]
        ties = sum(len(set(r)) < E for r in score.tolist())
        assert ties > B // 2
        _, _, _, idx = _head(logits, None, mask, k, bias=bias)
        assert np.array_equal(idx.cpu().numpy(), ridx), (E, k, mask is not None)
        if mask is None:
            assert idx[0].tolist() == list(range(k))


@gpu
def test_overflow_case_weights_are_finite():
    """Two picked experts 100 apart in raw logits, the bias making the smaller one the first pick: stabilised by the first pick, the
    other weight would be exp(100) = inf and the row NaN.  Also the mirrored row, and a three-pick row."""
    logits = np.array([[100.0, 0.0, -50.0, -60.0], [0.0, 100.0, -60.0, -50.0], [-30.0, 70.0, -50.0, -29.0]], np.float32)
    bias = np.array([0.0, 150.0, 0.0, 0.0], np.float32)
    for k in (2, 3):
        sparse, _, _, idx = _head(logits, None, None, k, bias=bias)
        got = idx.cpu().numpy().astype(np.int64)
        ridx, near = _ref_topk(logits, bias, k)
        assert not near.any() and np.array_equal(got, ridx)
        assert got[0, 0] == 1 and got[0, 1] == 0                 # the first pick is 100 below the second in raw value
        sp = sparse.cpu().numpy().astype(np.float64)
        assert np.isfinite(sp).all()
        ref, dmax = _ref_weights(logits, got)
        assert dmax.max() >= 100.0
        bound = (2.0 * (dmax[:, None] + 4.0) + k + 1) * U * ref + 2e-38
        assert bool((np.abs(sp - ref) <= bound).all()), (sp, ref)
        assert abs(sp[0, 0] - 1.0) <= 4 * U and abs(sp[1, 1] - 1.0) <= 4 * U


@gpu
@pytest.mark.parametrize("E,k", [(4, 2), (8, 1), (64, 2), (64, 64), (1, 1)])
def test_backward_is_the_fp64_gradient_with_idx_held_constant(E, k):
    from hdmoe_hip import ops
    for B in (63, 257):
        for masked in (False, True):
            logits, noise, mask, bias = _inputs(B, E, k, True, masked, 2)
            rng = np.random.default_rng(B + E + k)
            gs, gp, gx = (rng.standard_normal((B, E)).astype(np.float32) for _ in range(3))
            lt = _t(logits).requires_grad_(True)
            sparse, probs, xout, idx = ops.router_head(lt, _t(noise), _t(mask), k, sel_bias=_t(bias))
            (sparse * _t(gs) + probs * _t(gp) + xout * _t(gx)).sum().backward()
            torch.cuda.synchronize()
            got = lt.grad.cpu().numpy().astype(np.float64)
            x = _xout(logits, noise, mask).astype(np.float64)
            sel = idx.cpu().numpy().astype(np.int64)
            with np.errstate(invalid="ignore"):
                p = np.exp(x - x.max(1, keepdims=True))
                p = p / p.sum(1, keepdims=True)
            w, _ = _ref_weights(x.astype(np.float32), sel)
            picked = np.zeros((B, E), dtype=bool)
            picked[np.arange(B)[:, None], sel] = True
            ref = gx + p * (gp - (p * gp).sum(1, keepdims=True)) + np.where(picked, w * (gs - (w * gs * picked).sum(1, keepdims=True)), 0.0)
            if mask is not None:
                ref = np.where(mask == 0, 0.0, ref)
                assert bool((got[mask == 0] == 0).all())
                ok = mask.sum(1) > 0
            else:
                ok = np.ones(B, dtype=bool)
            tol = 4.0 * (E + 40) * U * (np.abs(gs).max() + np.abs(gp).max() + np.abs(gx).max())
            err = float(np.abs(got[ok] - ref[ok]).max())
            print(f"B={B} E={E} k={k} masked={masked}: max |dlogits - fp64| = {err:.3e} (bound {tol:.3e})")
            assert err <= tol


# ------------------------------------------------------------------------------------------------------------------ accumulators
@gpu
@pytest.mark.parametrize("E,k", EK)
def test_accumulators_equal_the_integer_reference(E, k):
    for B in BS:
        for masked in (False, True):
            load = torch.zeros(E, dtype=torch.int64, device=DEV)
            target = torch.zeros(E, dtype=torch.int64, device=DEV)
            want_l, want_t = [0] * E, [0] * E
            for call in range(2):                                # two calls in a row add up
                logits, noise, mask, bias = _inputs(B, E, k, True, masked, 3 + call)
                sparse, _, _, idx = _head(logits, noise, mask, k, bias=bias, accum=(load, target))
                l, t = _ref_counts(idx.cpu().numpy(), mask, B, E, k)
                want_l, want_t = [a + b for a, b in zip(want_l, l)], [a + b for a, b in zip(want_t, t)]
                assert load.tolist() == want_l and target.tolist() == want_t, (B, E, k, masked, call)
                # what is counted is what the dispatch routes: the pairs with a weight > 0
                assert l == (sparse > 0).sum(0).tolist()
                if mask is None:
                    assert sum(l) == B * k and all(v == B * (((k << (SHIFT + 1)) + E) // (2 * E)) for v in t)
                elif B > 2:
                    assert mask[0].sum() == 0 and mask[1].sum() == 1          # a_b = 0 and (for k > 1) a_b < k are among the rows
    # without the pair nothing is touched
    _head(logits, noise, mask, k, bias=bias)
    assert load.tolist() == want_l and target.tolist() == want_t


@gpu
def test_a_router_counts_only_when_it_trains():
    """Router._fwd hands the accumulators to the head in train mode with grad enabled, and never else."""
    import models.model_components as mc
    torch.manual_seed(3)
    r = mc.Router(in_channels=4, time_dim=6, top_k=2, num_experts=5).to(DEV)
    r.enable_balance()
    assert set(r._non_persistent_buffers_set) == {"balance_bias", "balance_load", "balance_target"}
    assert not any("balance" in key for key in r.state_dict())
    x, te = torch.randn(7, 4, 8, 8, device=DEV), torch.randn(7, 6, device=DEV)
    r.eval()
    r(x, te, None, 0.0)
    r.train()
    with torch.no_grad():
        r(x, te, None, 0.01)
    torch.cuda.synchronize()
    assert r.balance_load.tolist() == [0] * 5 and r.balance_target.tolist() == [0] * 5
    sparse, _, _ = r(x, te, None, 0.01)
    torch.cuda.synchronize()
    assert r.balance_load.tolist() == (sparse > 0).sum(0).tolist() and int(r.balance_load.sum()) == 14
    assert r.balance_target.tolist() == [7 * (((2 << (SHIFT + 1)) + 5) // 10)] * 5


# ------------------------------------------------------------------------------------------------------------------ the update
def _ref_update(bias, load, target, rate, bias_max):
    """fp32 numpy, the kernel's order: + rate * sign, minus the mean (an index-order sum), clamp.  Dyadic values: every step exact."""
    E = len(bias)
    sign = np.array([(t > (l << SHIFT)) - (t < (l << SHIFT)) for l, t in zip(load, target)], dtype=np.float32)
    v = (bias + np.float32(rate) * sign).astype(np.float32)
    s = np.float32(0)
    for i in range(E):
        s = np.float32(s + v[i])
    v = (v - np.float32(s / np.float32(E))).astype(np.float32)
    return np.minimum(np.maximum(v, np.float32(-bias_max)), np.float32(bias_max)).astype(np.float32)


@gpu
@pytest.mark.parametrize("E", [1, 4, 8, 64])
def test_update_kernel_against_numpy(E):
    from hdmoe_hip import ops
    rng = np.random.default_rng(E)
    rate, bias_max = 0.25, 0.5
    bias0 = (rng.integers(-8, 9, E) / 8.0).astype(np.float32)    # multiples of 1/8 in [-1, 1]
    if E > 1:                                                    # the clamp bites on both sides whatever the draw: the mean of the moved
        bias0[0], bias0[2] = -1.0, 1.0                           # values lies within +-0.6, these two move to -1.25 and 1.25
    load = [int(v) for v in rng.integers(0, 50, E)]
    rel = [(-1, 0, 1)[i % 3] for i in range(E)]                  # target below / equal to / above 2^20 * load
    target = [max((l << SHIFT) + s * int(rng.integers(1, 1 << 22)), 0) if s else (l << SHIFT) for l, s in zip(load, rel)]
    if E > 1:
        target[1] = load[1] << SHIFT                             # an exact tie whatever the draw
    want = _ref_update(bias0, load, target, rate, bias_max)
    signs = {(t > (l << SHIFT)) - (t < (l << SHIFT)) for l, t in zip(load, target)}
    assert E == 1 or signs == {-1, 0, 1}
    if E > 1:
        assert float(want.max()) == bias_max and float(want.min()) == -bias_max      # the clamp was reached on both sides
        assert len({float(v) for v in want}) > 2                                      # ... and not by everything
    for ok in (None, 1, 0):
        b = _t(bias0)
        l, t = _t(load, torch.int64), _t(target, torch.int64)
        ll, lt = torch.full((E,), -7, dtype=torch.int64, device=DEV), torch.full((E,), -7, dtype=torch.int64, device=DEV)
        okt = None if ok is None else torch.tensor([ok], dtype=torch.int32, device=DEV)
        ops.balance_bias_update(b, l, t, ll, lt, okt, rate, bias_max)
        torch.cuda.synchronize()
        got = b.cpu().numpy()
        if ok == 0:
            assert np.array_equal(got.view(np.int32), bias0.view(np.int32))           # bit for bit what it was
        else:
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (ok, got, want)
        assert ll.tolist() == load and lt.tolist() == target                          # the copies, always
        assert l.tolist() == [0] * E and t.tolist() == [0] * E                        # the clear, always
    # the re-centring alone: no clamp in reach, all signs +1 -> the bias keeps its (zero-mean) values
    if E > 1:
        z = (bias0 - bias0.mean(dtype=np.float32)).astype(np.float32) / 4
        b = _t(z)
        ops.balance_bias_update(b, _t([0] * E, torch.int64), _t([5] * E, torch.int64), ll, lt, None, rate, 8.0)
        assert np.array_equal(b.cpu().numpy(), _ref_update(z, [0] * E, [5] * E, rate, 8.0))
        assert float(np.abs(b.cpu().numpy() - z).max()) <= 2 ** -20


# ------------------------------------------------------------------------------------------------------------------ convergence
CONV = dict(B=256, E=4, k=2, rounds=200, rate=0.05, bias_max=8.0, offsets=(2.0, 0.5, -0.5, -2.0))


def _conv_inputs(seed, masked):
    c = CONV
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((c["B"], c["E"])) + np.array(c["offsets"])).astype(np.float32)        # fixed over the rounds
    mask = None
    if masked:                                                   # half the rows may not use expert 0
        mask = np.ones((c["B"], c["E"]), np.float32)
        mask[: c["B"] // 2, 0] = 0.0
    return logits, mask


@functools.lru_cache(maxsize=None)
def _simulate(seed, masked):
    """fp64 simulation of head + update over the device loop's inputs -> max_e load / target per round."""
    c = CONV
    logits, mask = _conv_inputs(seed, masked)
    B, E, k = c["B"], c["E"], c["k"]
    allowed, share = _shares(mask, B, E, k)
    target = np.array([sum(share[b] for b in range(B) if allowed[b, e]) for e in range(E)], dtype=np.float64)
    bias = np.zeros(E)
    ratios = []
    for r in range(c["rounds"]):
        x = logits.astype(np.float64)
        if mask is not None:
            x = np.where(mask == 0, -np.inf, x)
        idx = np.argsort(-(x + bias), axis=1, kind="stable")[:, :k]
        load = np.bincount(idx.ravel(), minlength=E).astype(np.float64)
        ratios.append(float((load * 2.0 ** SHIFT / target).max()))
        bias = bias + c["rate"] * np.sign(target - load * 2.0 ** SHIFT)
        bias = np.clip(bias - bias.mean(), -c["bias_max"], c["bias_max"])
    return ratios


CONV_CASES = [(seed, masked) for seed in (0, 1, 2) for masked in (False, True)]


@pytest.mark.parametrize("seed,masked", CONV_CASES)
def test_the_simulation_itself_converges(seed, masked):
    """CPU: 200 rounds at rate 0.05 bring max(load / target) from ~2 to under 1.10 over the last 20 rounds."""
    ratios = _simulate(seed, masked)
    print(f"seed {seed} masked {masked}: round 0 {ratios[0]:.3f}, last 20 max {max(ratios[-20:]):.3f}")
    assert ratios[0] > 1.5
    assert max(ratios[-20:]) < 1.10


@gpu
@pytest.mark.parametrize("seed,masked", CONV_CASES)
def test_device_loop_converges_like_the_simulation(seed, masked):
    """The device loop (fp32 bias, rate 0.05 not dyadic) may flip a near-tie row against the simulation: one row moves the ratio by
    ~1 / 128 = 0.008; the margin 0.05 allows about six."""
    from hdmoe_hip import ops
    c = CONV
    sim = _simulate(seed, masked)
    assert max(sim[-20:]) < 1.10
    logits, mask = _conv_inputs(seed, masked)
    E, k, R = c["E"], c["k"], c["rounds"]
    lg, mk = _t(logits), _t(mask)
    bias = torch.zeros(E, device=DEV)
    load, target = torch.zeros(E, dtype=torch.int64, device=DEV), torch.zeros(E, dtype=torch.int64, device=DEV)
    ll, lt = torch.zeros_like(load), torch.zeros_like(load)
    hist = torch.zeros(R, 2, E, dtype=torch.int64, device=DEV)
    for r in range(R):
        ops.router_head(lg, None, mk, k, sel_bias=bias, accum=(load, target))
        ops.balance_bias_update(bias, load, target, ll, lt, None, c["rate"], c["bias_max"])
        hist[r, 0].copy_(ll)
        hist[r, 1].copy_(lt)
    h = hist.cpu().numpy().astype(np.float64)
    ratios = (h[:, 0] * 2.0 ** SHIFT / h[:, 1]).max(1)
    print(f"seed {seed} masked {masked}: device round 0 {ratios[0]:.3f} (sim {sim[0]:.3f}), last 20 max {ratios[-20:].max():.3f} "
          f"(sim {max(sim[-20:]):.3f}), bias {bias.tolist()}")
    assert ratios[0] == sim[0]                                   # zero bias, the same inputs: the same routing
    assert ratios[-20:].max() <= max(sim[-20:]) + 0.05
