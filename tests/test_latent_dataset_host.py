"""The keyed permutation behind the device-resident dataset's epoch order, through its host entry point (csrc/keyed_perm.h,
hdmoe_dataset_perm): no device needed.  The reference is the contract of include/hdmoe.h in numpy -- eight Feistel rounds whose round
function is word 0 of a Philox4x32-10 block, then cycle walking -- over the numpy Philox of test_text_dropout.py, copied here so that the
file stands alone."""
import ctypes

import numpy as np
import pytest

SEED = 0x1234ABCD5678EF01
GOLDEN = 0x9E3779B97F4A7C15
PERM_SALT = 0xA0761D6478BD642F
M64 = (1 << 64) - 1
EINVAL = -1
NS = [1, 2, 3, 4, 5, 16, 17, 37, 255, 256, 257, 1000, 2040]


# ------------------------------------------------------------------------------------------------------------------ the reference
def philox_word0(c0, c1, key):
    """Word 0 of the Philox4x32-10 blocks (c0[j], c1, 0, 0) (Salmon et al., SC'11) under the 64-bit `key` (low word k0, high word k1)."""
    c = [np.asarray(c0, dtype=np.uint64), np.full(len(c0), c1, dtype=np.uint64), np.zeros(len(c0), np.uint64), np.zeros(len(c0), np.uint64)]
    k0, k1, lo = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0]


def perm_ref(seed, epoch, N, xs):
    """perm(seed, epoch, N, x) of include/hdmoe.h for every x of `xs`, int64."""
    k = max(2, int(N - 1).bit_length())
    k += k & 1
    h = np.uint64(k // 2)
    m = np.uint64((1 << (k // 2)) - 1)
    key = ((seed ^ PERM_SALT) + epoch * GOLDEN) & M64

    def rounds(y):
        L, R = y >> h, y & m
        for r in range(8):
            L, R = R, L ^ (philox_word0(R, r, key) & m)
        return (L << h) | R

    y = rounds(np.asarray(xs, dtype=np.uint64))
    while True:                                               # cycle walking, on the entries still outside [0, N)
        out = y >= np.uint64(N)
        if not out.any():
            return y.astype(np.int64)
        y[out] = rounds(y[out])


def perm_lib(seed, epoch, N, first=0, count=None):
    from hdmoe_hip import _lib
    count = N - first if count is None else count
    out = np.full(count + 2, -7, dtype=np.int32)              # two sentinels behind the window
    rc = _lib.lib().hdmoe_dataset_perm(out.ctypes.data, seed, epoch, N, first, count)
    assert rc == 0, rc
    assert (out[count:] == -7).all()
    return out[:count].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("N", NS)
def test_entry_point_equals_the_model_and_is_a_permutation(N):
    got = perm_lib(SEED, 3, N)
    assert np.array_equal(np.sort(got), np.arange(N))
    assert np.array_equal(got, perm_ref(SEED, 3, N, np.arange(N)))


@pytest.mark.parametrize("N,first,count", [(37, 5, 12), (37, 36, 1), (37, 37, 0), (2040, 1000, 1040), (257, 0, 1)])
def test_partial_window_is_a_slice_of_the_full_permutation(N, first, count):
    full = perm_lib(SEED, 3, N)
    assert np.array_equal(perm_lib(SEED, 3, N, first, count), full[first:first + count])


@pytest.mark.parametrize("N,x", [(10, 0), (10, 7), (1000, 0), (1000, 999)])
def test_one_position_is_uniform_over_the_epochs(N, x):
    """Epochs 0 .. 2999, the image of position x in 10 equal bins: chi-square against uniform below 27.88, the 0.1 % quantile at 9
    degrees of freedom.  (Four rounds instead of eight give 26.1 at (10, 7); the model of the eight-round construction gives 4.0, 11.4,
    7.8, 12.4 for these four cases.)  The library's values are compared with the model's on the way."""
    from hdmoe_hip import _lib
    fn = _lib.lib().hdmoe_dataset_perm
    out = np.zeros(1, dtype=np.int32)
    img = np.empty(3000, dtype=np.int64)
    for e in range(3000):
        assert fn(out.ctypes.data, SEED, e, N, x, 1) == 0
        img[e] = out[0]
    for e in (0, 1, 2999):
        assert img[e] == perm_ref(SEED, e, N, [x])[0]
    counts = np.bincount(img * 10 // N, minlength=10)
    chi2 = float(((counts - 300.0) ** 2 / 300.0).sum())
    print(f"N = {N}, x = {x}: chi-square {chi2:.2f}")
    assert chi2 < 27.88


def test_epochs_and_seeds_give_different_permutations():
    a = perm_lib(SEED, 0, 1000)
    assert not np.array_equal(a, perm_lib(SEED, 1, 1000))
    assert not np.array_equal(a, perm_lib(SEED + 1, 0, 1000))
    assert np.array_equal(a, perm_lib(SEED, 0, 1000))


def test_entry_point_rejects_bad_arguments():
    from hdmoe_hip import _lib
    fn = _lib.lib().hdmoe_dataset_perm
    out = np.full(8, -7, dtype=np.int32)
    ok = dict(out=out.ctypes.data, N=8, first=0, count=8)
    bad = [dict(out=None), dict(N=0), dict(N=-3), dict(N=1 << 31), dict(first=-1), dict(count=-1), dict(first=1), dict(count=9),
           dict(first=9, count=0)]
    for over in bad:
        a = dict(ok, **over)
        assert fn(a["out"], SEED, 0, a["N"], a["first"], a["count"]) == EINVAL, over
        assert (out == -7).all(), over
    assert fn(ok["out"], SEED, 0, (1 << 31) - 1, (1 << 31) - 9, 8) == 0       # the largest N, its last window
    assert ((out >= 0) & (out < (1 << 31) - 1)).all() and len(set(out.tolist())) == 8
