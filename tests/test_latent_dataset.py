"""The device-resident latent dataset (csrc/traingen.hip hdmoe_dataset_inputs / hdmoe_text_gather_dropout, ops.dataset_inputs,
ops.text_gather_dropout, Utils.utils.LatentDataset, DeviceInputs.generate_from / text_from, Trainer(dataset=...)): the step's items
against the numpy model of the keyed permutation, flips against a numpy Philox4x32-10, the posterior draw and the noise against
ops.randn_keyed, both access paths and their edges, the text gather bit for bit, the error paths, and the trainer eager and graphed.
The numpy Philox and permutation are those of test_text_dropout.py / test_latent_dataset_host.py (anchored to the library there), copied
here so that the file stands alone."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234ABCD5678EF01
GOLDEN = 0x9E3779B97F4A7C15
PERM_SALT = 0xA0761D6478BD642F
DATA_SALT = 0xE7037ED1A0B428DB
M64 = (1 << 64) - 1
SENTINEL = -7.0
PAD = 64
SMIN, SMAX = 0.002, 80.0


# ------------------------------------------------------------------------------------------------------------------ the reference
def philox4x32_10(c0, c1, key):
    """Blocks (c0[j], c1, 0, 0) of Philox4x32-10 (Salmon et al., SC'11) under the 64-bit `key` (low word k0, high word k1): (n, 4) uint32."""
    c = [np.asarray(c0, dtype=np.uint64), np.full(len(c0), c1, dtype=np.uint64), np.zeros(len(c0), np.uint64), np.zeros(len(c0), np.uint64)]
    k0, k1, lo = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def u01(w):
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def perm_ref(seed, epoch, N, xs):
    """perm(seed, epoch, N, x) of include/hdmoe.h for every x of `xs`, int64."""
    k = max(2, int(N - 1).bit_length())
    k += k & 1
    h, m = np.uint64(k // 2), np.uint64((1 << (k // 2)) - 1)
    key = ((seed ^ PERM_SALT) + epoch * GOLDEN) & M64

    def rounds(y):
        L, R = y >> h, y & m
        for r in range(8):
            L, R = R, L ^ (philox4x32_10(R, r, key)[:, 0].astype(np.uint64) & m)
        return (L << h) | R

    y = rounds(np.asarray(xs, dtype=np.uint64))
    while True:
        out = y >= np.uint64(N)
        if not out.any():
            return y.astype(np.int64)
        y[out] = rounds(y[out])


@functools.lru_cache(maxsize=None)
def items_ref(data_seed, step, N, B, world, rank):
    spe = N // (B * world)
    epoch, pos = step // spe, step % spe
    return perm_ref(data_seed, epoch, N, pos * B * world + rank * B + np.arange(B))


def flips_ref(seed_rank, step, B, p):
    key = ((seed_rank ^ DATA_SALT) + (4 * step + 1) * GOLDEN) & M64
    return (u01(philox4x32_10(np.arange((B + 3) // 4), 0, key).reshape(-1)[:B]) < np.float32(p)).astype(np.float32)


def keep_ref(seed, step, B, p):
    key = (seed + (4 * step + 3) * GOLDEN) & M64
    return (~(u01(philox4x32_10(np.arange((B + 3) // 4), 1, key).reshape(-1)[:B]) < np.float32(p))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ helpers
def _padded(shape, dtype, sentinel=SENTINEL):
    """A tensor of `shape` at the front of a sentinel-filled flat buffer that is PAD elements longer: (view, flat)."""
    n = int(np.prod(shape))
    flat = torch.full((n + PAD,), sentinel, dtype=dtype, device=DEV)
    return flat[:n].view(shape), flat


def _tail_untouched(view, flat, sentinel=SENTINEL):
    return bool((flat[view.numel():] == sentinel).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@functools.lru_cache(maxsize=None)
def _table(N, chw, dtype):
    """(mean, std) of the dataset, made once per shape and storage type and never written: std in [0.1, 1.1)."""
    g = torch.Generator(device=DEV).manual_seed(3)
    mean = (0.5 * torch.randn((N,) + chw, device=DEV, generator=g)).to(dtype)
    std = (0.1 + torch.rand((N,) + chw, device=DEV, generator=g)).to(dtype)
    return mean, std


def _centers(E=4):
    return torch.linspace(0, 1, E, dtype=torch.float32, device=DEV)


GEN = dict(sigma_min=SMIN, sigma_max=SMAX, p_mean=-0.4, p_std=1.0, extreme_prob=0.5, unet_bw=0.3, vit_bw=0.3, min_active=1, zeta=0.25)


def _run(mean, std, B, step, *, seed=SEED, data_seed=SEED, world=1, rank=0, scale=1.0, p_flip=0.0, E=4):
    """ops.dataset_inputs into sentinel-padded buffers: (dict of views, dict of flat buffers)."""
    from hdmoe_hip import ops
    chw = tuple(mean.shape[1:])
    spec = {"x": ((B,) + chw, torch.float32), "x0": ((B,) + chw, torch.float32), "sigma": ((B, 1, 1, 1), torch.float32),
            "unet_mask": ((B, E), torch.float32), "vit_mask": ((B, E), torch.float32), "zeta": ((1,), torch.float32),
            "src": ((B,), torch.int32), "item": ((B,), torch.int32), "flip": ((B,), torch.float32)}
    v, f = {}, {}
    for k, (shape, dt) in spec.items():
        v[k], f[k] = _padded(shape, dt, -7 if dt == torch.int32 else SENTINEL)
    cen = _centers(E)
    ops.dataset_inputs(v["x"], v["x0"], v["sigma"], v["unet_mask"], v["vit_mask"], v["zeta"], v["src"], v["item"], v["flip"], mean, std, cen, cen,
                       seed, data_seed, step, world=world, rank=rank, scale=scale, p_flip=p_flip, **GEN)
    return v, f


def _follows(out, base, mult, eps_ref):
    """out = base + mult eps_ref in the tolerance form of test_train_inputs.py's noise check: the recovered draw within
    1e-5 max(|eps_ref|, 1) / min(|mult|, 1), or -- where mult eps_ref is below the last bits of base -- out within 1e-6 of the sum."""
    out, base, mult = out.double(), base.double(), mult.double()
    eps = (out - base) / mult
    tol = 1e-5 * eps_ref.abs().clamp(min=1.0) / mult.abs().clamp(max=1.0)
    ok = (eps - eps_ref).abs() <= tol
    ref = base + mult * eps_ref
    under = (mult * eps_ref).abs() < 2.0 ** -20 * base.abs()
    ok |= under & ((out - ref).abs() <= 1e-6 * ref.abs())
    return bool(ok.all()), float(((eps - eps_ref).abs() / tol).max())


# ------------------------------------------------------------------------------------------------------------------ the contract
# (N, B, (C,H,W)): one item; two steps per epoch with an item dropped; the 16-byte path; chw % 4 == 0 with W % 4 != 0 (scalar path: a
# vector would straddle rows); one vector per row; a batch that is no multiple of 4 with one step per epoch; the LDS limit B = 4096.
SHAPES = [(1, 1, (3, 3, 3)), (5, 2, (3, 3, 3)), (37, 6, (4, 16, 16)), (37, 6, (4, 8, 6)), (37, 6, (4, 4, 4)), (300, 250, (4, 16, 16)),
          (4096, 4096, (3, 3, 3))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,B,chw", SHAPES, ids=[f"N{s[0]}-B{s[1]}-{'x'.join(map(str, s[2]))}" for s in SHAPES])
def test_batch_follows_the_contract(N, B, chw, dtype):
    """flip in {0, 0.5, 1} x with / without std x scale in {1, 0.09}, at steps on both sides of an epoch boundary."""
    from hdmoe_hip import ops
    mean, std = _table(N, chw, dtype)
    spe = N // B
    steps = sorted({0, spe - 1, spe, 2 * spe + 1})             # the last step of epoch 0, the first of epoch 1, one inside epoch 2
    combos = [(p, ws, sc) for p in (0.0, 0.5, 1.0) for ws in (True, False) for sc in (1.0, 0.09)]
    worst = 0.0
    for n, (p_flip, with_std, scale) in enumerate(combos):
        for step in (steps if n < 2 else steps[n % len(steps):][:1]):      # every step for the first two combinations, one for the others
            v, f = _run(mean, std if with_std else None, B, step, scale=scale, p_flip=p_flip)
            torch.cuda.synchronize()
            where = (p_flip, with_std, scale, step)
            for k in v:
                assert _tail_untouched(v[k], f[k], -7 if v[k].dtype == torch.int32 else SENTINEL), (k, where)
            item = torch.from_numpy(items_ref(SEED, step, N, B, 1, 0)).to(DEV)
            assert torch.equal(v["item"].long(), item), where
            flip = torch.from_numpy(flips_ref(SEED, step, B, p_flip)).to(DEV)
            assert torch.equal(v["flip"], flip), where
            if p_flip in (0.0, 1.0):
                assert float(flip.sum()) == B * p_flip
            fl = flip.bool().view(B, 1, 1, 1)
            gm = torch.where(fl, mean[item].flip(-1), mean[item]).float()
            if with_std:
                gs = torch.where(fl, std[item].flip(-1), std[item]).float()
                eps_p = ops.randn_keyed(v["x0"], SEED ^ DATA_SALT, 4 * step).double()
                ok, r = _follows(v["x0"].double() / float(np.float32(scale)), gm, gs, eps_p)
                worst = max(worst, r)
                assert ok, where
            elif scale == 1.0:
                assert torch.equal(_bits(v["x0"]), _bits(gm)), where                    # the gathered, mirrored mean bit for bit
            else:
                want = gm.double() * float(np.float32(scale))
                assert bool(((v["x0"].double() - want).abs() <= 1e-6 * want.abs()).all()), where
            eps = ops.randn_keyed(v["x"], SEED, 4 * step).double()
            ok, r = _follows(v["x"], v["x0"], v["sigma"], eps)
            worst = max(worst, r)
            assert ok, where
    print(f"max |draw - ref| / tol = {worst:.3e}")


def test_generator_outputs_equal_train_inputs_bit_for_bit():
    """sigma, both masks, zeta, src -- and x, given the same x0 bits -- are ops.train_inputs' for the same (seed_rank, step), on both
    access paths, for a rank-mixed seed; item and flip do not touch them."""
    from hdmoe_hip import ops
    seed_rank = (SEED + 3 * GOLDEN) & M64
    for N, B, chw in ((300, 250, (4, 16, 16)), (37, 6, (4, 8, 6)), (37, 6, (3, 3, 3))):
        mean, std = _table(N, chw, torch.float32)
        for step in (0, 11):
            v, _ = _run(mean, std, B, step, seed=seed_rank, data_seed=SEED, world=1, rank=0, scale=0.09, p_flip=0.5)
            t = {k: torch.full_like(v[k], -7) for k in ("x", "sigma", "unet_mask", "vit_mask", "zeta", "src")}
            cen = _centers()
            ops.train_inputs(t["x"], t["sigma"], t["unet_mask"], t["vit_mask"], t["zeta"], t["src"], v["x0"].contiguous(), cen, cen, seed_rank, step, **GEN)
            for k in t:
                assert torch.equal(_bits(v[k]), _bits(t[k])), (k, N, B, chw, step)


def test_ranks_hold_disjoint_slices_of_one_epoch():
    """(N, B, world) = (37, 6, 2): the 2 x 3 x 6 = 36 items of one epoch are distinct, the next epoch's order differs; the ranks' seeds
    differ (rank mixed in), the data seed does not."""
    N, B, world = 37, 6, 2
    mean, _ = _table(N, (3, 3, 3), torch.float32)
    epochs = []
    for e in range(2):
        seen = []
        for pos in range(3):
            for rank in range(world):
                step = 3 * e + pos
                v, _ = _run(mean, None, B, step, seed=(SEED + rank * GOLDEN) & M64, data_seed=SEED, world=world, rank=rank)
                got = v["item"].cpu().numpy().astype(np.int64)
                assert np.array_equal(got, items_ref(SEED, step, N, B, world, rank)), (step, rank)
                seen += got.tolist()
        assert len(set(seen)) == 36 and min(seen) >= 0 and max(seen) < N
        epochs.append(seen)
    assert epochs[0] != epochs[1]


def test_flip_rate():
    """B = 4096 at p = 0.5: 2048 +- 5 sqrt(4096 / 4) = 2048 +- 160."""
    mean, _ = _table(4096, (3, 3, 3), torch.float32)
    v, _ = _run(mean, None, 4096, 2, p_flip=0.5)
    n = int(v["flip"].sum())
    print(f"{n} of 4096 flipped")
    assert abs(n - 2048) <= 160 and bool(((v["flip"] == 0) | (v["flip"] == 1)).all())


# ------------------------------------------------------------------------------------------------------------------ text
TEXT = [(1, None, (7,), torch.bfloat16), (37, None, (7,), torch.bfloat16), (3, "index", (7,), torch.bfloat16),
        (1, None, (77, 8), torch.float32), (37, None, (77, 8), torch.float32), (3, "index", (77, 8), torch.float32)]


@pytest.mark.parametrize("K,index,row,dtype", TEXT, ids=[f"K{c[0]}-{c[1] or 'direct'}-{'x'.join(map(str, c[2]))}-{c[3]}".replace("torch.", "") for c in TEXT])
def test_text_rows_and_keep(K, index, row, dtype):
    """Rows as bits for p in {0, 0.3, 1} with and without a null row; keep equal to ops.text_dropout's for the same key."""
    from hdmoe_hip import ops
    N, B, step = 37, 6, 11
    g = torch.Generator(device=DEV).manual_seed(5)
    table = torch.randn((K,) + row, device=DEV, generator=g).to(dtype)
    null = torch.randn(row, device=DEV, generator=g).to(dtype)
    tidx = torch.randint(0, K, (N,), device=DEV, generator=g).to(torch.int32) if index else None
    item = torch.from_numpy(items_ref(SEED, step, N, B, 1, 0)).to(device=DEV, dtype=torch.int32)
    t = tidx.long()[item.long()] if index else (torch.zeros(B, dtype=torch.long, device=DEV) if K == 1 else item.long())
    for p in (0.0, 0.3, 1.0):
        for with_null in (True, False):
            out, out_flat = _padded((B,) + row, dtype)
            keep, keep_flat = _padded((B,), torch.float32)
            ops.text_gather_dropout(out, keep, table, tidx, item, null if with_null else None, SEED, step, p, N)
            torch.cuda.synchronize()
            want_keep = torch.from_numpy(keep_ref(SEED, step, B, p)).to(DEV)
            assert torch.equal(keep, want_keep), (p, with_null)
            k2 = torch.empty(B, device=DEV)
            dummy = torch.zeros((B,) + row, dtype=dtype, device=DEV)
            ops.text_dropout(torch.empty_like(dummy), k2, dummy, None, SEED, step, p)
            assert torch.equal(keep, k2), (p, with_null)
            sub = null if with_null else torch.zeros(row, dtype=dtype, device=DEV)
            want = torch.where(want_keep.bool().view(B, *([1] * len(row))), table[t], sub.unsqueeze(0).expand((B,) + row))
            assert torch.equal(_bits(out), _bits(want)), (p, with_null)
            assert _tail_untouched(out, out_flat) and _tail_untouched(keep, keep_flat)
            if p == 0.0:
                assert float(keep.sum()) == B
            if p == 1.0:
                assert float(keep.sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ errors
def test_ops_errors_raise_before_anything_is_written():
    from hdmoe_hip import ops
    N, B, chw, E = 37, 6, (4, 4, 4), 4
    mean, std = _table(N, chw, torch.float32)
    f = dict(device=DEV)

    def good():
        return dict(x=torch.full((B,) + chw, SENTINEL, **f), x0=torch.full((B,) + chw, SENTINEL, **f), sigma=torch.full((B, 1, 1, 1), SENTINEL, **f),
                    unet_mask=torch.full((B, E), SENTINEL, **f), vit_mask=torch.full((B, E), SENTINEL, **f), zeta=torch.full((1,), SENTINEL, **f),
                    src=torch.full((B,), -7, dtype=torch.int32, **f), item=torch.full((B,), -7, dtype=torch.int32, **f),
                    flip=torch.full((B,), SENTINEL, **f), mean=mean, std=std, world=1, rank=0, scale=1.0, p_flip=0.5, step=0, min_active=1)

    shared = torch.full((2 * B * 64,), SENTINEL, **f)
    bad = {
        "mean not 4-D": dict(mean=mean.view(N, -1)), "mean dtype": dict(mean=mean.half(), std=None),
        "mean not contiguous": dict(mean=_table(N, (4, 4, 4), torch.float32)[0].transpose(2, 3), std=None),
        "std shape": dict(std=std[:N - 1]), "std dtype": dict(std=std.bfloat16()),
        "x0 shape": dict(x0=torch.full((B, 4, 4, 5), SENTINEL, **f)), "x shape": dict(x=torch.full((B + 1,) + chw, SENTINEL, **f)),
        "x dtype": dict(x=torch.full((B,) + chw, SENTINEL, dtype=torch.bfloat16, **f)),
        "x in x0's storage": dict(x=shared[:B * 64].view((B,) + chw), x0=shared[B * 64:].view((B,) + chw)),
        "item dtype": dict(item=torch.full((B,), -7, dtype=torch.int64, **f)), "item shape": dict(item=torch.full((B + 1,), -7, dtype=torch.int32, **f)),
        "flip dtype": dict(flip=torch.full((B,), -7, dtype=torch.int32, **f)), "flip not contiguous": dict(flip=torch.full((2 * B,), SENTINEL, **f)[::2]),
        "N < B world": dict(world=7, rank=0), "rank >= world": dict(world=2, rank=2), "rank < 0": dict(rank=-1), "world < 1": dict(world=0),
        "p_flip < 0": dict(p_flip=-0.1), "p_flip > 1": dict(p_flip=1.5), "p_flip nan": dict(p_flip=float("nan")), "scale nan": dict(scale=float("nan")),
        "step < 0": dict(step=-1), "min_active > E": dict(min_active=5),
    }
    outs = ("x", "x0", "sigma", "unet_mask", "vit_mask", "zeta", "src", "item", "flip")
    for name, over in bad.items():
        a = dict(good(), **over)
        snap = {k: a[k].clone() for k in outs}
        cen = _centers(E)
        with pytest.raises(ValueError):
            ops.dataset_inputs(a["x"], a["x0"], a["sigma"], a["unet_mask"], a["vit_mask"], a["zeta"], a["src"], a["item"], a["flip"], a["mean"],
                               a["std"], cen, cen, SEED, SEED, a["step"], world=a["world"], rank=a["rank"], scale=a["scale"], p_flip=a["p_flip"],
                               **dict(GEN, min_active=a["min_active"]))
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(a[k], snap[k]), (name, k)
    # B > 4096: the library's own limit
    big = torch.zeros(4097, 1, 1, 1, **f)
    a = good()
    with pytest.raises(ValueError):
        ops.dataset_inputs(torch.zeros(4097, 1, 1, 1, **f), torch.zeros(4097, 1, 1, 1, **f), torch.zeros(4097, 1, 1, 1, **f), torch.zeros(4097, E, **f),
                           torch.zeros(4097, E, **f), a["zeta"], torch.zeros(4097, dtype=torch.int32, **f), torch.zeros(4097, dtype=torch.int32, **f),
                           torch.zeros(4097, **f), big, None, _centers(E), _centers(E), SEED, SEED, 0, **GEN)
    assert float(a["zeta"]) == SENTINEL

    # ---- text
    row, K = (4, 8), 3
    table = torch.randn((K,) + row, **f)
    tidx = torch.zeros(N, dtype=torch.int32, **f)
    item = torch.zeros(B, dtype=torch.int32, **f)
    tgood = lambda: dict(out=torch.full((B,) + row, SENTINEL, **f), keep=torch.full((B,), SENTINEL, **f), table=table, tidx=tidx, item=item,
                         null=None, p=0.3, n=N, step=0)
    tshared = torch.full((2 * B * 32,), SENTINEL, **f)
    tbad = {
        "K neither 1 nor N without an index": dict(tidx=None), "table dtype": dict(table=table.double()), "table 1-D": dict(table=torch.randn(5, **f)),
        "table not contiguous": dict(table=torch.randn(K, 8, 4, **f).transpose(1, 2)), "out shape": dict(out=torch.full((B, 8, 4), SENTINEL, **f)),
        "out dtype": dict(out=torch.full((B,) + row, SENTINEL, dtype=torch.bfloat16, **f)), "keep shape": dict(keep=torch.full((B + 1,), SENTINEL, **f)),
        "item dtype": dict(item=item.long()), "item 2-D": dict(item=item.view(B, 1)), "index dtype": dict(tidx=tidx.long()), "index shape": dict(tidx=tidx[:N - 1]),
        "null shape": dict(null=torch.randn(4, 4, **f)), "null dtype": dict(null=torch.randn(row, **f).bfloat16()),
        "out in the table's storage": dict(table=tshared[:B * 32].view((B,) + row), out=tshared[B * 32:].view((B,) + row), n=B, tidx=None),
        "p < 0": dict(p=-0.1), "p > 1": dict(p=1.5), "p nan": dict(p=float("nan")), "step < 0": dict(step=-1), "n_items < 1": dict(n=0, tidx=None),
    }
    for name, over in tbad.items():
        a = dict(tgood(), **over)
        snap_out, snap_keep = a["out"].clone(), a["keep"].clone()
        with pytest.raises(ValueError):
            ops.text_gather_dropout(a["out"], a["keep"], a["table"], a["tidx"], a["item"], a["null"], SEED, a["step"], a["p"], a["n"])
        torch.cuda.synchronize()
        assert torch.equal(_bits(a["out"]), _bits(snap_out)) and torch.equal(a["keep"], snap_keep), name
    a = tgood()                                               # and the same call without a fault goes through
    ops.text_gather_dropout(a["out"], a["keep"], table, tidx, item, None, SEED, 0, 0.3, N)
    assert not bool((a["keep"] == SENTINEL).any())


def test_latent_dataset_checks_its_arguments():
    from Utils.utils import LatentDataset
    N = 5
    mean, std = torch.zeros(N, 4, 4, 4), torch.ones(N, 4, 4, 4)
    text = torch.zeros(3, 5, 8)
    idx = torch.tensor([0, 1, 2, 2, 0], dtype=torch.int32)
    bad = [dict(mean=mean[0]), dict(mean=mean.half()), dict(mean=mean[:0]), dict(mean=mean, std=std[:, :2]), dict(mean=mean, std=std.bfloat16()),
           dict(mean=mean, scale=float("inf")), dict(mean=mean, flip=-0.1), dict(mean=mean, flip=1.1), dict(mean=mean, flip=float("nan")),
           dict(mean=mean, text=text), dict(mean=mean, text=text, text_index=idx.long()), dict(mean=mean, text=text, text_index=idx[:4]),
           dict(mean=mean, text_index=idx), dict(mean=mean, text=torch.zeros(3)), dict(mean=mean, text=text.double(), text_index=idx),
           dict(mean=mean, text=text, text_index=torch.tensor([0, 1, 3, 2, 0], dtype=torch.int32)),       # 3 is no row of a 3-row table
           dict(mean=mean, text=text, text_index=torch.tensor([0, -1, 2, 2, 0], dtype=torch.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            LatentDataset(**kw)
    ds = LatentDataset(mean, std, scale=0.09, flip=0.5, text=text, text_index=idx)
    assert len(ds) == N and ds.mean.is_cuda and ds.std.is_cuda and ds.text.is_cuda and ds.text_index.is_cuda
    assert ds.mean.is_contiguous() and ds.text_index.dtype == torch.int32
    assert LatentDataset(mean.bfloat16(), text=text[:1]).mean.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ DeviceInputs
def _device_inputs(seed, rank, cond_dropout=0.0):
    from Utils import configs
    from Utils.utils import DeviceInputs, MaskGenerator, ZetaScheduler
    mc = configs.mask_configs
    mcfg = dict(configs.model_configs, total_steps=4)
    mk = lambda attr, rng: MaskGenerator(expert_attributes=mc[attr], p_mean=mc["p_mean"], p_std=mc["p_std"], total_steps=mcfg["total_steps"],
                                         min_active=mc["min_active"], step_size=mc["step_size"], max_bandwidth=mc["max_BW"], bandwidth=mc["BW"],
                                         strat_band=mc["strat_band"], noise_range=mc[rng])
    zc = configs.zeta_configs
    zs = ZetaScheduler(total_steps=zc["total_schedule_steps"], max_zeta=zc["max_zeta"], min_zeta=zc["min_zeta"], strategy=zc["strategy"],
                       warmup_ratio=zc["warmup_ratio"])
    return DeviceInputs(mcfg, mc, zc, mk("unet_attr", "unet_noise_range"), mk("vit_attr", "vit_noise_range"), zs, seed=seed, rank=rank,
                        cond_dropout=cond_dropout)


def test_device_inputs_generate_from_and_text_from():
    from Utils.utils import LatentDataset
    N, B, chw = 37, 6, (4, 16, 16)
    mean, std = _table(N, chw, torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(9)
    text = torch.randn(3, 5, 32, device=DEV, generator=g)
    idx = torch.randint(0, 3, (N,), device=DEV, generator=g).to(torch.int32)
    ds = LatentDataset(mean, std, scale=0.09, flip=0.5, text=text, text_index=idx)
    di = _device_inputs(SEED, 1, cond_dropout=0.3)
    assert di.data_seed == SEED and di.seed == (SEED + GOLDEN) & M64
    a = di.generate_from(ds, 7, B, world=2, rank=1)
    assert set(a) == {"sigma", "x", "unet_mask", "vit_mask", "zeta", "src", "x0", "item", "flip"}
    ptrs = {k: t.data_ptr() for k, t in a.items()}
    first = {k: t.clone() for k, t in a.items()}
    assert np.array_equal(first["item"].cpu().numpy(), items_ref(SEED, 7, N, B, 2, 1))
    assert torch.equal(first["flip"].cpu(), torch.from_numpy(flips_ref(di.seed, 7, B, 0.5)))
    out, keep = di.text_from(ds, 7)
    assert torch.equal(keep.cpu(), torch.from_numpy(keep_ref(di.seed, 7, B, 0.3)))
    rows = torch.where(keep.bool().view(B, 1, 1), text[idx.long()[first["item"].long()]], torch.zeros_like(out))
    assert torch.equal(out, rows)
    mine = torch.full_like(out, SENTINEL)
    assert di.text_from(ds, 7, out=mine)[0] is mine and torch.equal(mine, rows)
    c = di.generate_from(ds, 8, B, world=2, rank=1)
    assert {k: t.data_ptr() for k, t in c.items()} == ptrs and not torch.equal(c["item"], first["item"])
    again = di.generate_from(ds, 7, B, world=2, rank=1)
    for k in first:
        assert torch.equal(_bits(again[k]), _bits(first[k])), k
    for kw in (dict(batch_size=5), dict(batch_size=B, world=7), dict(batch_size=B, world=2, rank=2), dict(batch_size=0)):
        with pytest.raises(ValueError):
            di.generate_from(ds, 7, **kw)
    with pytest.raises(ValueError):
        _device_inputs(SEED, 0).text_from(ds, 0)              # no generate_from before it
    with pytest.raises(ValueError):
        di.text_from(LatentDataset(mean), 7)                  # a dataset without text


# ------------------------------------------------------------------------------------------------------------------ the trainer
TINY = dict(img_resolution=16, internal_channels=8, time_emb_dim=16, text_emb_dim=32, VIT_num_blocks=1, VIT_patch_sizes=[2, 4, 4, 8],
            VIT_num_groups=2, VIT_num_heads=2, VIT_emb_size=8, Unet_num_blocks=1, Unet_model_channels=8, log_var_channels=8, top_k=2)
TSEED = 0x0BADC0FFEE123457
TN, TB = 20, 8                                                # two steps per epoch, four items dropped


def _no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model


def _dataset():
    from Utils.utils import LatentDataset
    mean, std = _table(TN, (4, 16, 16), torch.float32)
    text = torch.randn(TN, 5, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    return LatentDataset(mean, std, scale=1.0, flip=0.5, text=text)


def _tiny_trainer(**kw):
    """The small config-2 model of test_trainer_cond_dropout.py: zeta 0 and every dropout p = 0, so a step is a function of its weights
    and inputs alone."""
    from Utils import configs, training
    from models import model_config2
    mcfg = dict(configs.model_configs, **TINY, total_steps=10)
    zeta = dict(configs.zeta_configs, total_schedule_steps=4, max_zeta=0.0, min_zeta=0.0, warmup_ratio=0.0)
    torch.manual_seed(0)
    model = _no_dropout(model_config2.preconditioned_HDMOEM(**configs.model_kwargs(mcfg)).to(DEV).train())
    return training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, zeta, **kw)


def _follow(dst, src):
    from hdmoe_hip import bank
    dst.model.load_state_dict(src.model.state_dict())
    bank.note_weights_changed()


@pytest.fixture
def bf16():
    import hdmoe_hip
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    yield
    hdmoe_hip.set_compute_dtype(torch.float32)


def _snap(tr, res):
    return dict(item=res["item"].clone(), flip=res["flip"].clone(), sigma=res["sigma"].clone(), x0=tr.inputs.data_buf["x0"].clone(),
                loss=res["loss"]["loss"].detach().clone())


def test_trainer_eager_same_seed_same_data_resume_and_train_steps(bf16):
    """Two eager trainers with one seed, three steps side by side (the second starts every step from the first one's weights and the same
    library seed: the backward's fp32 atomics make free-running weights differ in the last bits, test_trainer_cond_dropout.py's
    _lockstep): identical item / flip / loss, the items those of the numpy model, crossing an epoch at step 2.  A fresh trainer set to
    step 1 reproduces step 1's data; train_steps(trainer, 3) makes three steps over the same items."""
    import hdmoe_hip
    from Utils import training
    ds = _dataset()
    A, B = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED), _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED)
    assert A.device_inputs and not A.graphed
    steps = []
    for step in range(3):
        _follow(B, A)
        got = []
        for tr in (A, B):
            hdmoe_hip.manual_seed(99)
            res = tr.train_step()
            assert {"loss", "out_model", "sigma", "item", "flip"} <= set(res) and "text_keep" not in res
            got.append(_snap(tr, res))
        torch.cuda.synchronize()
        a, b = got
        print(f"step {step}: loss {float(a['loss']):.9g} / {float(b['loss']):.9g}, items {a['item'].tolist()}")
        assert torch.equal(a["item"], b["item"]) and torch.equal(a["flip"], b["flip"]) and torch.equal(a["loss"], b["loss"]), step
        assert np.array_equal(a["item"].cpu().numpy(), items_ref(TSEED, step, TN, TB, 1, 0)), step
        steps.append(a)
    assert len(set(steps[0]["item"].tolist() + steps[1]["item"].tolist())) == 2 * TB        # one epoch: no item twice
    assert A.step_idx == 3
    T = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED)
    T.step_idx = 1
    r = _snap(T, T.train_step())
    assert T.step_idx == 2
    for k in ("item", "flip", "sigma", "x0"):
        assert torch.equal(r[k], steps[1][k]), k
    C = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED)
    seen = []
    training.train_steps(C, 3, on_step=lambda s, res: seen.append((s, res["item"].clone())))
    assert C.step_idx == 3 and [s for s, _ in seen] == [0, 1, 2]
    assert all(torch.equal(it, steps[s]["item"]) for s, it in seen)
    # cond_dropout rides on the gather: text_keep is the keyed decision of the step, the items are unchanged
    D = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED, cond_dropout=0.5)
    res = D.train_step()
    assert torch.equal(res["text_keep"].cpu(), torch.from_numpy(keep_ref(TSEED, 0, TB, 0.5))) and 0 < float(res["text_keep"].sum()) < TB
    assert torch.equal(res["item"], steps[0]["item"])
    rows = torch.where(res["text_keep"].bool().view(TB, 1, 1), ds.text[res["item"].long()], torch.zeros(TB, 5, 32, device=DEV))
    assert torch.equal(D.inputs.text, rows)
    # the argument rules
    lat, text = torch.zeros(TB, 4, 16, 16, device=DEV), torch.zeros(TB, 5, 32, device=DEV)
    with pytest.raises(ValueError):
        C.train_step(lat, text)
    assert C.step_idx == 3
    plain = _tiny_trainer(device_inputs=True, seed=TSEED)
    with pytest.raises(ValueError):
        plain.train_step()
    with pytest.raises(ValueError):
        training.train_steps(plain, 3)
    for kw in (dict(dataset=ds), dict(dataset=ds, batch_size=0), dict(dataset=ds, batch_size=TN + 1), dict(batch_size=TB),
               dict(dataset="flowers", batch_size=TB)):
        with pytest.raises(ValueError):
            _tiny_trainer(seed=TSEED, **kw)
    from Utils.utils import LatentDataset
    with pytest.raises(ValueError):
        _tiny_trainer(seed=TSEED, dataset=LatentDataset(ds.mean), batch_size=TB)               # no text rows


def test_trainer_graphed_matches_eager_and_resumes(bf16):
    """graphed=True over the generator's own buffers against the eager dataset trainer: the same item / flip each step, loss and
    gradients within test_trainer_graphed.py's bf16 bounds for that pair (loss 1e-3 relative, every gradient tensor 1e-2 of its largest
    entry; the eager side starts every step from the graphed side's weights and has run twice before, as there).  The captured step reads x0 where the generator writes it.  A fresh graphed trainer set
    to step 1 reproduces step 1's item, flip, sigma and x0."""
    ds = _dataset()
    G = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED, graphed=True)
    E = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED)
    for _ in range(2):
        E.train_step()
    E.step_idx = 0
    inner = G._build_staged

    def build(*a):                                            # the capture's warm-up runs renormalise G's weights: E copies them after it
        inner(*a)
        _follow(E, G)

    G._build_staged = build
    steps = []
    for step in range(3):
        _follow(E, G)
        g = _snap(G, G.train_step())
        gg = {n: p.grad.detach().clone() for n, p in G.model.named_parameters() if p.grad is not None}
        e = _snap(E, E.train_step())
        torch.cuda.synchronize()
        print(f"step {step}: loss graphed {float(g['loss']):.7g} eager {float(e['loss']):.7g}, items {g['item'].tolist()}")
        for k in ("item", "flip", "sigma", "x0"):
            assert torch.equal(g[k], e[k]), (step, k)
        assert np.array_equal(g["item"].cpu().numpy(), items_ref(TSEED, step, TN, TB, 1, 0)), step
        assert abs(float(g["loss"]) - float(e["loss"])) <= 1e-3 * abs(float(e["loss"])) + 1e-6
        bad, worst = [], 0.0
        for n, p in E.model.named_parameters():
            if p.grad is not None:
                scale, err = float(p.grad.abs().max()), float((gg[n] - p.grad).abs().max())
                worst = max(worst, err / (scale + 1e-30))
                if err > 1e-2 * scale + 1e-7:
                    bad.append((n, err, scale))
        print(f"step {step}: worst gradient error / max|ref| = {worst:.3e} over {len(gg)} tensors")
        assert not bad and len(gg) > 100, (bad[:5], len(gg))
        rows = ds.text[g["item"].long()]
        assert torch.equal(G._text, rows), step               # the static text buffer holds the step's rows
        steps.append(g)
    assert G._lat.data_ptr() == G.inputs.data_buf["x0"].data_ptr() and G.inputs.text is None
    assert G.step_idx == 3 and not torch.equal(steps[0]["item"], steps[1]["item"])
    R = _tiny_trainer(dataset=ds, batch_size=TB, seed=TSEED, graphed=True)
    R.step_idx = 1
    r = _snap(R, R.train_step())
    for k in ("item", "flip", "sigma", "x0"):
        assert torch.equal(r[k], steps[1][k]), k
