"""Text-conditioning dropout on the device (csrc/traingen.hip hdmoe_text_dropout, ops.text_dropout): the keep decision against a numpy
Philox4x32-10 that is first anchored to the library's own keyed normals, the rows bit for bit, both access paths and their edges, the
untouched tails, determinism, the drop rate, the shuffle stream left alone, the error paths."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x1234ABCD5678EF01
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
PAD = 64
SENTINEL = -7.0


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
    """common.h's u01 in float32: the + 0.5f rounds (to even) for 24-bit words >= 2^23, here as there."""
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def stream_key(seed, ctr):
    return (seed + ctr * GOLDEN) & M64


def draws(seed, step, B, c1):
    """u01 of word i % 4 of block (i / 4, c1) under the r = 3 key of `step`: c1 = 1 the drop draws d_i, c1 = 0 the shuffle keys k_i."""
    return u01(philox4x32_10(np.arange((B + 3) // 4), c1, stream_key(seed, 4 * step + 3)).reshape(-1)[:B])


def keep_ref(seed, step, B, p):
    return (~(draws(seed, step, B, 1) < np.float32(p))).astype(np.float32)


@gpu
def test_numpy_philox_reproduces_the_librarys_keyed_normals():
    """The anchor: the reference's blocks (c1 = 0) through randn4's Box-Muller are ops.randn_keyed, to the 1e-5 (relative to
    max(|ref|, 1)) that test_train_inputs.py uses for the same comparison.  Nothing below is judged by an unanchored generator."""
    from hdmoe_hip import ops
    for seed, stage in ((SEED, 0), (SEED, 4 * 11 + 3), (7, 2)):
        r = philox4x32_10(np.arange(256), 0, stream_key(seed, stage))
        u = u01(r)
        a0, a1 = np.sqrt(-2.0 * np.log(u[:, 0].astype(np.float64))), np.sqrt(-2.0 * np.log(u[:, 2].astype(np.float64)))
        t0, t1 = (np.float32(6.28318530717958648) * u[:, 1]).astype(np.float64), (np.float32(6.28318530717958648) * u[:, 3]).astype(np.float64)
        ref = np.stack([a0 * np.cos(t0), a0 * np.sin(t0), a1 * np.cos(t1), a1 * np.sin(t1)], axis=1).reshape(-1)
        got = ops.randn_keyed(torch.empty(1024, device=DEV), seed, stage).double().cpu().numpy()
        err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
        print(f"seed {seed:#x} stage {stage}: max err {err.max():.3e}")
        assert err.max() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ the contract
def _padded(shape, dtype, offset=0):
    """A tensor of `shape` inside a sentinel-filled flat buffer that is PAD elements longer (`offset` elements in front): (view, flat)."""
    n = int(np.prod(shape))
    flat = torch.full((offset + n + PAD,), SENTINEL, dtype=dtype, device=DEV)
    return flat[offset:offset + n].view(shape), flat


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _data(B, row, dtype, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    text = torch.randn((B,) + tuple(row), device=DEV, generator=g).to(dtype)
    null = torch.randn(tuple(row), device=DEV, generator=g).to(dtype)
    return text, null


def _check(B, row, dtype, with_null, p, step, offset=0):
    from hdmoe_hip import ops
    text, null = _data(B, row, dtype)
    null = null if with_null else None
    out, out_flat = _padded((B,) + tuple(row), dtype, offset)
    keep, keep_flat = _padded((B,), torch.float32)
    ops.text_dropout(out, keep, text, null, SEED, step, p)
    torch.cuda.synchronize()
    want_keep = torch.from_numpy(keep_ref(SEED, step, B, p)).to(DEV)
    assert torch.equal(keep, want_keep), (p, step, int((keep != want_keep).sum()))
    sub = null if with_null else torch.zeros(tuple(row), dtype=dtype, device=DEV)
    want = torch.where(want_keep.bool().view(B, *([1] * len(row))), text, sub.unsqueeze(0).expand_as(text))
    assert torch.equal(_bits(out), _bits(want)), (p, step)
    n = out.numel()
    assert bool((out_flat[:offset] == SENTINEL).all()) and bool((out_flat[offset + n:] == SENTINEL).all())
    assert bool((keep_flat[B:] == SENTINEL).all())
    # the same (seed, step) again, bit for bit
    out2, _ = _padded((B,) + tuple(row), dtype, offset)
    keep2, _ = _padded((B,), torch.float32)
    ops.text_dropout(out2, keep2, text, null, SEED, step, p)
    assert torch.equal(keep2, keep) and torch.equal(_bits(out2), _bits(out))
    return keep


# (B, row shape, dtype, null row given, element offset of `out` inside its allocation).  A row is cut into equal segments of at most
# 4096 accesses, one per workgroup and trip, at most 2048 workgroups.  Beyond the listed shapes: a row of 4099 fp32 = two segments of the
# element path, the second one short; 2049 rows = two trips with a last workgroup that makes one; and a 16-byte-multiple row whose `out`
# is only 4-byte aligned (the alignment half of the 16-byte condition).
CASES = [(1, (77, 768), torch.float32, True, 0),          # the real text shape
         (6, (77, 768), torch.float32, True, 0),          # the real row, 16-byte path: 4 segments of 3696 accesses, 14.4 per thread
         (6, (77, 768), torch.float32, False, 0),         # ... null = None: zeros
         (6, (3, 5), torch.float32, True, 0),             # 60-byte rows: element path, rows not 16-byte aligned
         (250, (7, 6), torch.bfloat16, True, 0),          # 84-byte rows, 2-byte elements
         (250, (7, 6), torch.bfloat16, False, 0),
         (256, (32,), torch.float16, True, 0),            # 2-D text, 64-byte rows: 16-byte path, a fraction of one segment
         (4096, (3, 5), torch.float32, True, 0),          # more rows than workgroups in the grid (2048): two trips each
         (3, (4099,), torch.float32, True, 0),
         (2049, (3,), torch.float16, False, 0),
         (6, (4, 4), torch.float32, True, 1)]
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
IDS = [f"B{c[0]}-{'x'.join(map(str, c[1]))}-{_DT[c[2]]}-{'null' if c[3] else 'zeros'}-off{c[4]}" for c in CASES]


@gpu
@pytest.mark.parametrize("B,row,dtype,with_null,offset", CASES, ids=IDS)
def test_rows_and_keep_follow_the_contract(B, row, dtype, with_null, offset):
    for step in (0, 11):
        for p in (0.0, 0.1, 0.5, 1.0):
            keep = _check(B, row, dtype, with_null, p, step, offset)
            if p == 0.0:
                assert float(keep.sum()) == B
            if p == 1.0:                                      # u01 == 1.0f needs the one word in 2^24: not under this seed (the reference says so)
                assert float(keep_ref(SEED, step, B, p).sum()) == 0 and float(keep.sum()) == 0


@gpu
def test_keep_varies_with_step_and_seed():
    from hdmoe_hip import ops
    B = 4096
    text, null = _data(B, (3, 5), torch.float32)
    out = torch.empty_like(text)
    got = {}
    for seed, step in ((SEED, 0), (SEED, 1), (SEED + 1, 0)):
        keep = torch.empty(B, device=DEV)
        ops.text_dropout(out, keep, text, null, seed, step, 0.5)
        assert torch.equal(keep.cpu(), torch.from_numpy(keep_ref(seed, step, B, 0.5)))
        got[(seed, step)] = keep
    assert not torch.equal(got[(SEED, 0)], got[(SEED, 1)]) and not torch.equal(got[(SEED, 0)], got[(SEED + 1, 0)])


@gpu
def test_drop_rate():
    """N = 16 x 4096 draws at p = 0.1: the count within 5 sigma = 5 sqrt(N p (1 - p)) = 384 of N p.  The reference itself is held to the
    bound first (it is: 6589 drops under this seed, computed on the host when the test was written)."""
    from hdmoe_hip import ops
    B, p, steps = 4096, 0.1, 16
    n = B * steps
    ref = sum(int(B - keep_ref(SEED, s, B, p).sum()) for s in range(steps))
    assert abs(ref - n * p) <= 384, ref
    text, null = _data(B, (32,), torch.float16)
    out, keep, dropped = torch.empty_like(text), torch.empty(B, device=DEV), 0
    for s in range(steps):
        ops.text_dropout(out, keep, text, null, SEED, s, p)
        dropped += int(B - keep.sum())
    print(f"dropped {dropped} of {n} (reference {ref}, expected {n * p:.1f} +- 384)")
    assert abs(dropped - n * p) <= 384 and dropped == ref


@gpu
def test_shuffle_stream_is_left_alone():
    """The drop draws share the r = 3 key with the shuffle keys (c1 = 1 against c1 = 0): train_inputs' src for the same (seed, step) is
    the rank of the reference's c1 = 0 draws, before and after a text_dropout call."""
    from hdmoe_hip import ops
    B, E, step = 250, 4, 11
    f = dict(dtype=torch.float32, device=DEV)
    x0 = torch.zeros(B, 3, 3, 3, **f)
    cen = torch.linspace(0, 1, E, **f)

    def src():
        b = dict(x=torch.empty_like(x0), sigma=torch.empty(B, 1, 1, 1, **f), um=torch.empty(B, E, **f), vm=torch.empty(B, E, **f),
                 zeta=torch.empty(1, **f), src=torch.empty(B, dtype=torch.int32, device=DEV))
        ops.train_inputs(b["x"], b["sigma"], b["um"], b["vm"], b["zeta"], b["src"], x0, cen, cen, SEED, step, sigma_min=0.002, sigma_max=80.0,
                         p_mean=-0.4, p_std=1.0, extreme_prob=0.5, unet_bw=0.3, vit_bw=0.3, min_active=1, zeta=0.0)
        return b["src"].cpu()

    before = src()
    text, null = _data(B, (7, 6), torch.bfloat16)
    ops.text_dropout(torch.empty_like(text), torch.empty(B, device=DEV), text, null, SEED, step, 0.5)
    after = src()
    assert torch.equal(before, after)
    k = draws(SEED, step, B, 0)
    rank = np.empty(B, dtype=np.int64)
    rank[np.argsort(k, kind="stable")] = np.arange(B)         # ties: the lower position first
    assert np.array_equal(before.numpy().astype(np.int64), rank)
    assert not np.array_equal(draws(SEED, step, B, 0), draws(SEED, step, B, 1))


# ------------------------------------------------------------------------------------------------------------------ errors
@gpu
def test_errors_raise_before_anything_is_written():
    from hdmoe_hip import ops
    B, row = 6, (4, 8)
    text, null = _data(B, row, torch.float32)
    ok_keep = lambda: torch.full((B,), SENTINEL, device=DEV)
    ok_out = lambda: torch.full((B,) + row, SENTINEL, device=DEV)
    shared = torch.full((2 * B * 32,), SENTINEL, device=DEV)
    bad = {
        "out not contiguous": dict(out=torch.full((B, 8, 4), SENTINEL, device=DEV).transpose(1, 2)),
        "text not contiguous": dict(text=torch.randn(B, 8, 4, device=DEV).transpose(1, 2)),
        "keep not contiguous": dict(keep=torch.full((2 * B,), SENTINEL, device=DEV)[::2]),
        "null not contiguous": dict(null=torch.randn(8, 4, device=DEV).t()),
        "out dtype": dict(out=torch.full((B,) + row, SENTINEL, device=DEV, dtype=torch.bfloat16)),
        "out shape": dict(out=torch.full((B, 8, 4), SENTINEL, device=DEV)),
        "null shape": dict(null=torch.randn(4, 4, device=DEV)),
        "null is a batch": dict(null=torch.randn((B,) + row, device=DEV)),
        "null dtype": dict(null=null.to(torch.bfloat16)),
        "keep shape": dict(keep=torch.full((B, 1), SENTINEL, device=DEV)),
        "keep dtype": dict(keep=torch.full((B,), SENTINEL, device=DEV, dtype=torch.float64)),
        "out is text": dict(out=text),
        "out in text's storage": dict(text=shared[:B * 32].view((B,) + row), out=shared[B * 32:].view((B,) + row)),
        "p < 0": dict(p=-0.1), "p > 1": dict(p=1.5), "p nan": dict(p=float("nan")),
    }
    for name, over in bad.items():
        a = dict(out=ok_out(), keep=ok_keep(), text=text, null=null, p=0.5)
        a.update(over)
        snap_out, snap_keep = a["out"].clone(), a["keep"].clone()
        with pytest.raises(ValueError):
            ops.text_dropout(a["out"], a["keep"], a["text"], a["null"], SEED, 0, a["p"])
        torch.cuda.synchronize()
        assert torch.equal(a["out"], snap_out) and torch.equal(a["keep"], snap_keep), name
    out, keep = ok_out(), ok_keep()                           # and the same call without a fault goes through
    ops.text_dropout(out, keep, text, null, SEED, 0, 0.5)
    assert not bool((out == SENTINEL).any()) and not bool((keep == SENTINEL).any())


def test_c_entry_rejects_bad_arguments_without_a_device():
    """HDMOE_EINVAL (-1) of include/hdmoe.h, returned before anything is launched: the pointers are never followed."""
    from hdmoe_hip import _lib
    fn = _lib.lib().hdmoe_text_dropout
    ok = dict(out=0x1000, keep=0x2000, text=0x3000, null=None, B=4, row=8, eb=4, p=0.5)
    bad = [dict(out=None), dict(keep=None), dict(text=None), dict(B=0), dict(row=0), dict(eb=1), dict(eb=8), dict(p=-0.1), dict(p=1.5),
           dict(p=float("nan")), dict(out=0x3000)]
    for over in bad:
        a = dict(ok, **over)
        assert fn(a["out"], a["keep"], a["text"], a["null"], 1, 0, a["B"], a["row"], a["eb"], a["p"], None) == -1, over
