"""hdmoe_mt_stats (csrc/optim.hip) against fp64 numpy over the same fp32 values: per-group {sum, sum of squares, min, max} over the finite
elements, the non-finite and element counts, the verdict and its counters, the bit-identity of the total sum of squares with
hdmoe_mt_sumsq, the argument errors and the empty table."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 4096
SIZES = (1, 3, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)
ODD_VIEW = 5003                                     # elements of the tensor that is a view one element into a larger buffer
MULTI = SIZES.index(3 * 4096 + 5)                   # the multi-chunk tensor
NGROUPS = (1, 3, 64)
U = 2.0 ** -24                                      # fp32 unit roundoff


def additions(nchunks):
    """Additions on the longest path of the kernel's summation order, read off csrc/optim.hip:
      mt_stats_kernel        a thread adds its 4096 / 256 = 16 elements in order, wave_sum adds 6 times (xor butterfly over 64 lanes),
                             block_stats adds the 4 wave values in order to 0.f (block_sum's tree)                         16 + 6 + 4
      mt_stats_final_kernel  a thread adds its ceil(nchunks / 1024) chunk partials in order, wave_sum 6, block_stats the 16 wave values
                                                                                                      ceil(nchunks / 1024) + 6 + 16
    plus 1 for the rounding of v * v where the compiler does not fuse it into the accumulation."""
    return 16 + 6 + 4 + math.ceil(nchunks / 1024) + 6 + 16 + 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import hdmoe_hip
    hdmoe_hip.lib()


@pytest.fixture(scope="module")
def bag():
    """Device tensors p and g of every size, filled differently and at different scales; host fp32 copies."""
    gen = torch.Generator().manual_seed(11)
    sizes = SIZES + (ODD_VIEW,)
    scales = [10.0 ** (i - 4) for i in range(len(sizes))]
    host_p = [s * torch.randn(n, generator=gen) for n, s in zip(sizes, scales)]
    host_g = [0.37 * s * (torch.randn(n, generator=gen) + 0.25) for n, s in zip(sizes, reversed(scales))]

    def to_dev(host):
        buf = torch.zeros(ODD_VIEW + 8, device=DEV)
        out = [h.to(DEV) for h in host[:-1]] + [buf[1:1 + ODD_VIEW]]
        out[-1].copy_(host[-1])
        assert out[-1].data_ptr() % 16 != 0
        return out

    return {"p": to_dev(host_p), "g": to_dev(host_g), "host_p": [h.numpy() for h in host_p], "host_g": [h.numpy() for h in host_g],
            "sizes": sizes}


def table(bag, ngroups):
    from hdmoe_hip.optim import _Table
    groups = [i % ngroups for i in range(len(bag["sizes"]))]
    return _Table([(p, g, None, None, grp) for p, g, grp in zip(bag["p"], bag["g"], groups)]), groups


class Out:
    def __init__(self, ngroups, sentinel=False):
        R = ngroups + 1
        self.stats = torch.full((R, 4), -7.5 if sentinel else 0.0, dtype=torch.float32, device=DEV)
        self.counts = torch.full((R, 2), -3, dtype=torch.int64, device=DEV)
        self.ok = torch.full((1,), -5, dtype=torch.int32, device=DEV)
        self.counters = torch.tensor([0, 0, 0, -1], dtype=torch.int64, device=DEV)

    def host(self):
        torch.cuda.synchronize()
        return self.stats.cpu().numpy(), self.counts.cpu().numpy(), int(self.ok.item()), self.counters.cpu().tolist()


def run(tab, ngroups, which=0, step=0, out=None, verdict=True):
    from hdmoe_hip._lib import call
    out = out or Out(ngroups)
    ws = torch.empty(6 * tab.n, dtype=torch.float32, device=DEV)
    call("hdmoe_mt_stats", out.stats, out.counts, out.ok if verdict else None, out.counters if verdict else None, tab.descs, tab.chunks,
         tab.n, ngroups, which, step, ws)
    return out


def reference(arrays, groups, ngroups):
    """fp64 rows over fp32 arrays: (sum, sumsq, min, max, sum |v|, sum v^2 as the error scales), counts; last row = total."""
    rows, counts = [], []
    for g in list(range(ngroups)) + [None]:
        vals = [a for a, grp in zip(arrays, groups) if g is None or grp == g]
        v = np.concatenate(vals).astype(np.float64) if vals else np.zeros(0)
        fin = v[np.isfinite(v)]
        rows.append((fin.sum(), (fin * fin).sum(), np.float32(fin.min()) if fin.size else np.float32(np.inf),
                     np.float32(fin.max()) if fin.size else np.float32(-np.inf), np.abs(fin).sum()))
        counts.append((v.size - fin.size, v.size))
    return rows, counts


def check(out, arrays, groups, ngroups, nchunks, what):
    stats, counts, ok, _ = out.host()
    rows, cnt = reference(arrays, groups, ngroups)
    k = additions(nchunks)
    worst = 0.0
    for r, (s, sq, mn, mx, sabs) in enumerate(rows):
        assert tuple(counts[r]) == cnt[r], (what, r, counts[r], cnt[r])
        assert stats[r, 2] == mn and stats[r, 3] == mx, (what, r, stats[r], mn, mx)
        es, eq = abs(float(stats[r, 0]) - s), abs(float(stats[r, 1]) - sq)
        if sabs > 0:
            worst = max(worst, es / (k * U * sabs), eq / (k * U * sq))
        assert es <= k * U * sabs, (what, r, "sum", es, k * U * sabs)
        assert eq <= k * U * sq, (what, r, "sumsq", eq, k * U * sq)
    bad = cnt[-1][0]
    assert ok == (1 if bad == 0 and np.isfinite(np.float32(rows[-1][1])) else 0), (what, ok, bad)
    return worst


# ------------------------------------------------------------------------------------------------------------ clean data
@pytest.mark.parametrize("ngroups", NGROUPS)
def test_clean_rows_match_fp64_and_the_total_is_sumsq_bit_for_bit(bag, ngroups):
    from hdmoe_hip._lib import call
    tab, groups = table(bag, ngroups)
    out = run(tab, ngroups)
    worst = check(out, bag["host_g"], groups, ngroups, tab.n, f"clean, {ngroups} groups")
    print(f"{ngroups} groups, {tab.n} chunks: worst error / (k u sum|term|) = {worst:.3f} with k = {additions(tab.n)}")
    assert out.host()[2] == 1
    ss = torch.empty(1, dtype=torch.float32, device=DEV)
    call("hdmoe_mt_sumsq", ss, tab.descs, tab.chunks, tab.n, tab.ws)
    assert torch.equal(out.stats[ngroups, 1:2], ss), (out.stats[ngroups, 1].item(), ss.item())
    again = run(tab, ngroups)                                            # two runs are bit-identical
    assert torch.equal(again.stats.view(torch.int32), out.stats.view(torch.int32)) and torch.equal(again.counts, out.counts)


def test_which_reads_the_right_array(bag):
    tab, groups = table(bag, 3)
    g, p = run(tab, 3, which=0), run(tab, 3, which=1)
    check(g, bag["host_g"], groups, 3, tab.n, "which = grad")
    check(p, bag["host_p"], groups, 3, tab.n, "which = param")
    assert not torch.equal(g.stats, p.stats)


# ------------------------------------------------------------------------------------------------------------ poisoned data
SPOTS = [(SIZES.index(4097), 0), (MULTI, 4095), (MULTI, 4096), (SIZES.index(257), 256), (SIZES.index(1), 0)]
POISON = [float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("ngroups", NGROUPS)
def test_poisoned_elements_are_counted_and_left_out(bag, ngroups):
    tab, groups = table(bag, ngroups)
    plans = [[(t, e, v)] for t, e in SPOTS for v in POISON]              # each alone ...
    plans.append([(t, e, POISON[i % 3]) for i, (t, e) in enumerate(SPOTS)])     # ... and all together
    for plan in plans:
        host = [a.copy() for a in bag["host_g"]]
        try:
            for t, e, v in plan:
                host[t][e] = v
                bag["g"][t][e] = v
            out = run(tab, ngroups)
            check(out, host, groups, ngroups, tab.n, f"poison {plan}, {ngroups} groups")
            stats, counts, ok, counters = out.host()
            assert ok == 0 and counts[ngroups, 0] == len(plan)
            assert np.isfinite(stats[ngroups, :2]).all()
            assert counters == [1, 1, 1, 0]
        finally:
            for t, e, _ in plan:
                bag["g"][t][e] = float(bag["host_g"][t][e])
    torch.cuda.synchronize()
    for d, h in zip(bag["g"], bag["host_g"]):                            # the shared bag is left as it was
        assert np.array_equal(d.cpu().numpy(), h)


def test_overflow_of_finite_elements_gives_a_bad_verdict():
    from hdmoe_hip.optim import _Table
    p = [torch.zeros(n, device=DEV) for n in (CHUNK + 3, 7)]
    g = [torch.zeros(n, device=DEV) for n in (CHUNK + 3, 7)]
    g[0][5], g[1][2] = 1.5e19, 1.5e19                                    # 2.25e38 each: finite squares, a sum past fp32's 3.4e38
    tab = _Table([(a, b, None, None, i) for i, (a, b) in enumerate(zip(p, g))])
    stats, counts, ok, counters = run(tab, 2, step=9).host()
    assert counts[:, 0].tolist() == [0, 0, 0] and counts[:, 1].tolist() == [CHUNK + 3, 7, CHUNK + 10]
    assert np.isfinite(stats[:2, 1]).all() and np.isinf(stats[2, 1]) and ok == 0
    assert counters == [1, 1, 1, 9]


# ------------------------------------------------------------------------------------------------------------ verdict counters
def test_counters_over_ok_bad_bad_ok(bag):
    tab, _ = table(bag, 3)
    out = Out(3)
    seen = []
    for step, bad in enumerate([False, True, True, False]):
        if bad:
            bag["g"][MULTI][CHUNK] = float("nan")
        try:
            run(tab, 3, step=step, out=out)
            seen.append((out.host()[2], out.host()[3]))
        finally:
            bag["g"][MULTI][CHUNK] = float(bag["host_g"][MULTI][CHUNK])
    assert [s[0] for s in seen] == [1, 0, 0, 1]
    assert seen[2][1] == [3, 2, 2, 2]                                    # behind the third pass: two in a row
    assert seen[3][1] == [4, 2, 0, 2]
    quiet = run(tab, 3, step=50, verdict=False)                          # statistics only: ok and counters are not touched
    assert quiet.host()[2] == -5 and quiet.host()[3] == [0, 0, 0, -1]


# ------------------------------------------------------------------------------------------------------------ errors, empty table
def test_every_einval_case_leaves_the_outputs_untouched(bag):
    from hdmoe_hip._lib import call
    tab, _ = table(bag, 3)
    ws = torch.empty(6 * tab.n, dtype=torch.float32, device=DEV)
    for case in ("stats", "counts", "ngroups0", "ngroups65", "which-1", "which2"):
        out = Out(64, sentinel=True)
        before = [t.clone() for t in (out.stats, out.counts, out.ok, out.counters)]
        args = [out.stats, out.counts, out.ok, out.counters, tab.descs, tab.chunks, tab.n, 3, 0, 0, ws]
        if case == "stats":
            args[0] = None
        elif case == "counts":
            args[1] = None
        elif case.startswith("ngroups"):
            args[7] = int(case[7:])
        else:
            args[8] = int(case[5:])
        with pytest.raises(RuntimeError, match="invalid argument"):
            call("hdmoe_mt_stats", *args)
        torch.cuda.synchronize()
        for a, b in zip(before, (out.stats, out.counts, out.ok, out.counters)):
            assert torch.equal(a, b), case


def test_empty_table_gives_the_documented_values():
    from hdmoe_hip._lib import call
    out = Out(3, sentinel=True)
    call("hdmoe_mt_stats", out.stats, out.counts, out.ok, out.counters, None, None, 0, 3, 0, 4, None)
    stats, counts, ok, counters = out.host()
    assert np.array_equal(stats, np.tile(np.array([0.0, 0.0, np.inf, -np.inf], dtype=np.float32), (4, 1)))
    assert not counts.any() and ok == 1 and counters == [1, 0, 0, -1]
