"""Autograd-aware wrappers over the HIP kernels (one torch.autograd.Function per fused op).

Layout contract of this module: activation tensors are contiguous channel-last -- spatial ``(N, H, W, C)``,
token ``(N, S, C)`` or matrix ``(M, C)`` -- in float32 or bfloat16.  "Vector path" tensors (per-sample scalars,
``(B, F)`` embeddings, parameters and their gradients) are float32.  PyTorch is used for memory (``torch.empty`` /
``zeros``), views and autograd bookkeeping only; every arithmetic op below is a call into libhdmoe_hip.so.
"""
from __future__ import annotations

import ctypes
import functools
import math
import numbers
from typing import Optional, Sequence, Tuple, Union

import torch

from . import bank as _bank
from ._lib import dtype_code_cast  # noqa: F401
from ._lib import BF16, _int_array, call, dtype_code, lib

Tensor = torch.Tensor

# C-ABI constants (include/hdmoe.h)
F32S = 2                                  # HDMOE_F32S, dtype code: fp32 tensors, split-bf16 arithmetic
ROUTE_CONV6S = 6                          # HDMOE_ROUTE_CONV_CONV6S


def _c(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    return t if t.is_contiguous() else t.contiguous()


def _dt(t: Tensor) -> int:
    return dtype_code(t.dtype)


def _f32(t: Tensor) -> Tensor:
    if t.dtype != torch.float32:
        raise TypeError("expected a float32 vector-path tensor")
    return _c(t)


_seed_state = {"seed": 0x5DEECE66D, "ctr": 0}

# Host-side counters of which fused paths a step took ("trunk": fused router trunk forward, "bwd6" / "bwd6s" / "pbwd": dgrad + wgrad in one
# launch (k x k / split-bf16 trunk / pointwise), "w6_defer": deferred wgrad6 reduction, "blk": fused Unet_block main branch): the parity tests assert that the path they
# pin to the reference is the one the benchmark times.
import collections as _collections
STATS = _collections.Counter()


def kernel_selections(reset: bool = False) -> dict:
    """The library's kernel-selection counters (include/hdmoe.h HDMOE_SEL_*): {"conv7_32": n, "bwd7_32_wgrad8": n, ...}, lower-case
    names without the prefix.  They count launches where the host code enqueues them -- under graph capture at the capture, not at
    each replay.  ``reset``: zero them after the read."""
    import re
    from ._lib import HEADER_PATH
    names = {}
    for m in re.finditer(r"\bHDMOE_SEL_(\w+)\s*=\s*(\d+)", open(HEADER_PATH).read()):
        if m.group(1) != "COUNT":
            names[int(m.group(2))] = m.group(1).lower()
    n = lib().hdmoe_kernel_selections(None, 0, 0)
    assert sorted(names) == list(range(n)), "include/hdmoe.h HDMOE_SEL_* names and the library's counters disagree"
    arr = (ctypes.c_longlong * n)()
    lib().hdmoe_kernel_selections(ctypes.cast(arr, ctypes.c_void_p), n, 1 if reset else 0)
    return {names[i]: int(arr[i]) for i in range(n)}


def manual_seed(seed: int) -> None:
    """Seed of the device counter RNG used for dropout masks and router logit noise."""
    _seed_state["seed"] = int(seed) & 0xFFFFFFFFFFFF
    _seed_state["ctr"] = 0


def _next_seed() -> int:
    _seed_state["ctr"] += 1
    return ((_seed_state["seed"] * 0x9E3779B97F4A7C15) ^ (_seed_state["ctr"] * 0xD1B54A32D192ED03)) & 0xFFFFFFFFFFFFFFFF


def next_seed() -> int:
    """The next 64-bit value of the library's seed stream (manual_seed restarts it): one per dropout / noise launch, one per stochastic
    EDM_Sampler.sample() call on the device path."""
    return _next_seed()


_step_counters = {}

# Independent, launch-latency-bound branches of the model (the ViT experts) run on side streams beside the main stream's
# large launches; False serialises everything on the caller's stream.
SIDE_STREAMS = True
_side_pool = {}


def side_streams(device, n: int):
    key = torch.device(device)
    pool = _side_pool.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=key))
    return pool[:n]


def step_counter(device) -> Tensor:
    """Device-resident step counter mixed into every dropout / noise Philox key (see csrc/elementwise.hip: mix_seed)."""
    key = torch.device(device)
    t = _step_counters.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=key)
        _step_counters[key] = t
    return t


def advance_seed(device) -> None:
    """Call once per training step (inside the captured region when the step is a hipGraph)."""
    call("hdmoe_seed_advance", step_counter(device))


# =====================================================================================================
# MP_Conv: weight prep + implicit GEMM conv (+dgrad, wgrad)
# =====================================================================================================
# Optional per-launch timing of the GEMM-shaped kernels (bench.py's roofline leg): when PROFILE is a list, every
# hdmoe_conv_fwd / hdmoe_conv_wgrad launch is bracketed by events on the launch stream and logged with its shape.
PROFILE = None
# PROFILE_FUSED: the timed leg keeps the weight-bank path of the replayed step -- dgrad + wgrad in one launch (bwd6 / bwd6s), the fused
# Unet_block launch (blk6), the fused router trunk, deferred wgrad6 reductions -- and brackets THOSE launches with events
# (bench.py: roofline = the in-step dominant kernel).  False: every layer on its own unfused kernels (the round-1/2 leg).
PROFILE_FUSED = False
_spacer = None


def _prof_ok() -> bool:
    return PROFILE is None or PROFILE_FUSED


def _timed(kind: str, info, name: str, *args):
    """``info``: the launch's record, or a callable that makes it -- called only when PROFILE is on and the launch was made."""
    if PROFILE is None:
        return call(name, *args)
    # An event pair also spans the time the stream sits idle waiting for the host to enqueue the kernel.  A spacer launch in
    # front keeps the GPU busy while start event, kernel and end event are all enqueued, so the pair brackets the kernel alone.
    global _spacer
    if _spacer is None:
        _spacer = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    _spacer.zero_()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = call(name, *args)
    e.record()
    if rc == 0:
        PROFILE.append((kind, info() if callable(info) else info, s, e))
    return rc


def _route(query: str, n: int, *args) -> list:
    """The ``n`` route ints of a route query of the library (include/hdmoe.h: hdmoe_conv_fwd_route, hdmoe_conv_wgrad_route) -- the library
    alone decides which kernel a layer gets, this asks it.  Host-only: nothing is launched.  Lists go as host int arrays."""
    r = (ctypes.c_int * n)()
    conv = [ctypes.cast(_int_array(a), ctypes.c_void_p) if isinstance(a, (list, tuple)) else int(a) for a in args]
    if getattr(lib(), query)(ctypes.cast(r, ctypes.c_void_p), *conv) != 0:
        raise RuntimeError(f"{query}: the library refuses the layer")
    return list(r)


@functools.lru_cache(maxsize=None)
def _c7_min_images() -> int:
    """conv7's least number of images (csrc/conv7.hip), asked of the library once."""
    return lib().hdmoe_conv7_min_images()


# kernel names as csrc/ spells them, by HDMOE_ROUTE_CONV_* / HDMOE_ROUTE_WGRAD_* (include/hdmoe.h); r = the route array, b = its ints as bools
_FWD_KERNELS = ("conv_fwd_kernel<{t}, {r[1]}, {b[2]}>", "conv_fwd2_kernel<{t}, {r[1]}, {b[2]}>", "conv_fwd3_kernel<{t}, {r[1]}>",
                "conv_fwd5_kernel<{t}, {r[1]}, {b[3]}, {r[4]}>", "conv7_kernel<{r[1]}, {r[2]}, {b[3]}>", "conv6_bf16_kernel<{r[1]}, {r[2]}>",
                "conv6_split_kernel<{r[1]}>", "kgemm_kernel<{r[1]}>", "glin_f32_kernel<{r[1]}>", "none", "rowlin_f32_kernel")
_WGRAD_KERNELS = (None, "conv_wgrad_kernel<{t}>", "swg_f32_kernel", "towg_bf16_kernel", "lwg_{s}_kernel")


def _kernel_label(r, x: Tensor, wgrad: bool = False) -> str:
    """The kernel instantiation(s) that a route array of hdmoe_conv_fwd_route / hdmoe_conv_wgrad_route names, for tensors of ``x``'s type."""
    t, s = ("float", "f32") if x.dtype == torch.float32 else ("__bf16", "bf16")
    b = ["true" if v else "false" for v in r]
    if not wgrad:
        return _FWD_KERNELS[r[0]].format(t=t, r=r, b=b)
    if r[0]:
        return _WGRAD_KERNELS[r[0]].format(t=t, s=s)
    # conv_wgrad2_kernel<T, OT, MAXT, VEC>, one launch per pass of each kernel-size class: (passes, MAXT, OT, VEC) per class from r[2]
    return " + ".join(f"conv_wgrad2_kernel<{t}, {r[4 + 4 * k]}, {r[3 + 4 * k]}, {b[5 + 4 * k]}>" + (f" x {r[2 + 4 * k]} passes" if r[2 + 4 * k] > 1 else "")
                      for k in range(r[1]))


def _conv_record(x, seg, N, HW, O, I, khs, kws, dtype=None, **name) -> dict:
    return dict(dtype=dtype or str(x.dtype).replace("torch.", ""), seg=seg, N=N, HW=HW, O=O, I=I, taps=[a * b for a, b in zip(khs, kws)], **name)


def _fwd_record(x, w, y, res, alpha, beta, seg, G, wstride, N, H, W, Ho, Wo, I, Cphys, Ipad, O, Cstore, stride, ones, khs, kws, pts, pls, dtc) -> dict:
    """Shape record of one hdmoe_conv_fwd call, from its own arguments, with the kernel the library routes it to."""
    r = _route("hdmoe_conv_fwd_route", 5, N, H, W, Ho, Wo, I, Cphys, Ipad, O, Cstore, stride, ones, G, seg is not None, res is not None, wstride,
               khs, kws, pts, pls, dtc, all(t is None or t.data_ptr() % 16 == 0 for t in (x, w, y, res)))
    return _conv_record(x, seg, N, Ho * Wo, O, I, khs, kws, "split_bf16" if r[0] == ROUTE_CONV6S else None, fwd_name=_kernel_label(r, x))


def _kernel_hw(w: Tensor):
    if w.ndim == 4:
        return int(w.shape[2]), int(w.shape[3])
    if w.ndim == 2:
        return 1, 1
    raise ValueError(f"weight must be 2-D or 4-D, got {tuple(w.shape)}")


# Small learnable tensors (norm affines, biases, rel_pos_bias, alpha_txt): when the parameter already owns a gradient buffer (the
# flat DP buckets, or a .grad kept from the previous step) the backward kernels -- which accumulate anyway -- add straight into it
# and hand autograd None.  That is what the weight bank does for the conv weights; per step it removes a zero-fill and an
# AccumulateGrad add per parameter (~300 launches of ~5 us that the host enqueues one by one).


def _direct(p) -> bool:
    return (p is not None and p.is_leaf and p.requires_grad and p.grad is not None
            and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.shape == p.shape)



class _ZeroPool:
    """Zero-initialised scratch for the backward kernels that ACCUMULATE (atomics) into a fresh buffer: ~50 such buffers per step
    were 50 memset launches.  One persistent buffer per device, cleared by ONE memset at the start of a step (WeightBank.begin_step),
    handed out in 256-byte-aligned slices.  Only for tensors that never become a leaf's .grad (autograd may adopt those)."""

    def __init__(self, device, nbytes=32 << 20):
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.off = 0
        self.high = 0

    def reset(self):
        if self.high:
            self.buf[:(self.high + 255) // 256 * 256].view(torch.float32).zero_()      # (a byte-typed fill runs one byte per thread)
        self.off = self.high = 0

    def take(self, shape, dtype):
        n = 1
        for d in shape:
            n *= int(d)
        nb = n * torch.empty((), dtype=dtype).element_size()
        start = (self.off + 255) // 256 * 256
        if start + nb > self.buf.numel():
            return None
        self.off = start + nb
        self.high = max(self.high, self.off)
        return self.buf[start:start + nb].view(dtype).view(*shape)


_zero_pools = {}


def zero_pool_reset(device) -> None:
    pool = _zero_pools.get(torch.device(device))
    if pool is not None:
        pool.reset()


def _zeros(shape, dtype, device, pool_ok: bool = True) -> Tensor:
    """torch.zeros for accumulate-into scratch / non-leaf gradients, served from the per-step zero pool when possible
    (``pool_ok=False``: the buffer may become a leaf's .grad -- autograd adopts incoming gradients -- and must own its memory)."""
    device = torch.device(device)
    if pool_ok and device.type == "cuda":
        pool = _zero_pools.get(device)
        if pool is None:
            if torch.cuda.is_current_stream_capturing():
                return torch.zeros(shape, dtype=dtype, device=device)
            pool = _zero_pools[device] = _ZeroPool(device)
        t = pool.take(tuple(shape), dtype)
        if t is not None:
            return t
    return torch.zeros(shape, dtype=dtype, device=device)


class _FanoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n, scales):
        ctx.set_materialize_grads(False)
        ctx.scales = scales
        return tuple(x.view(x.shape) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        sc = ctx.scales or (1.0,) * len(gs)
        pairs = [(_c(g), float(s)) for g, s in zip(gs, sc) if g is not None]
        if not pairs:
            return None, None, None
        if len(pairs) == 1 and pairs[0][1] == 1.0:
            return pairs[0][0], None, None
        out = torch.empty_like(pairs[0][0])
        for i in range(0, len(pairs), 15):                    # 16 sources per launch (the running sum takes one slot)
            part = pairs[i:i + 15] if i == 0 else [(out, 1.0)] + pairs[i:i + 15]
            call("hdmoe_sum_n", out, [g for g, _ in part], [s for _, s in part], len(part), out.numel(), _dt(out))
        return out, None, None


def fanout(x: Tensor, n: int, scales=None):
    """n aliases of ``x`` for n consumers: their gradients are summed by ONE kernel in the backward (autograd's own accumulation is
    n - 1 separate add launches).  ``scales``: per-alias factors applied to the incoming gradients inside that sum (a consumer that
    hands back an unscaled gradient, mp_conv(res_grad_raw=True)).  The aliases must not be modified in place."""
    if n <= 1 or not (torch.is_tensor(x) and x.requires_grad):
        return tuple(x for _ in range(max(n, 1)))
    return _FanoutFn.apply(x, int(n), None if scales is None else tuple(float(v) for v in scales))


class _W6Arena:
    """Workspace of the DEFERRED wgrad6 reductions: every k x k layer of the weight bank keeps its partial slabs until the end of the
    backward pass, where one batched launch per 16 layers sums them (WeightBank._finish).  One bump-allocated buffer per device,
    rewound at the start of a step.  It starts at W6_ARENA_MB and is re-sized to the step's high-water mark at the
    next rewind outside a graph capture: a layer that does not fit meanwhile takes the non-deferred path (its own cached workspace)."""

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(W6_ARENA_MB << 18, dtype=torch.float32, device=device)
        self.off = 0
        self.want = 0                                        # floats the current step would have needed
        self.captured = False                                # a hipGraph capture handed out slices of the CURRENT buffer
        self._old = []                                       # outgrown buffers that a captured graph may still point into

    def take(self, nfloats):
        self.want = (self.want + 63) // 64 * 64 + nfloats    # advances whether or not the slice fits: the next rewind grows to it
        start = (self.off + 63) // 64 * 64
        if start + nfloats > self.buf.numel():
            if torch.cuda.is_current_stream_capturing():
                # the captured step would bake the slower non-deferred path in: say how to avoid it instead of degrading silently
                import warnings
                warnings.warn(f"hdmoe_hip: the deferred weight-gradient arena ({self.buf.numel() * 4 >> 20} MB) is too small for this step and cannot "
                              f"grow inside a hipGraph capture; run one eager step before capturing (this step needs >= "
                              f"{(self.want * 5 >> 20) + 1} MB)", RuntimeWarning, stacklevel=3)
            return None
        self.off = start + nfloats
        if torch.cuda.is_current_stream_capturing():
            self.captured = True
        return self.buf[start:start + nfloats]

    def rewind(self):
        if self.want > self.buf.numel() and not torch.cuda.is_current_stream_capturing():
            if self.captured:                                # only a buffer some captured graph points into has to stay alive
                self._old.append(self.buf)
            self.buf = torch.empty(int(self.want * 1.25) // 64 * 64 + 64, dtype=torch.float32, device=self.device)
            self.captured = False
        self.off = self.want = 0

    def release_old(self):
        """Drop the outgrown buffers (call once every graph captured before the last growth has been destroyed)."""
        self._old.clear()


_w6_arenas = {}
W6_ARENA_MB = 1024                                         # initial size of the deferred weight-gradient arena


def w6_arena_reset(device) -> None:
    a = _w6_arenas.get(torch.device(device))
    if a is not None:
        a.rewind()


_w6_ws = {}


def _w6_kib(G, N, H, W, I, O, khs, kws, dtc) -> int:
    """KiB of partial weight-gradient slabs a wgrad6-reduced launch of this layer needs (csrc/wgrad6.hip); 0 outside its domain."""
    return lib().hdmoe_conv_wgrad6_ws_kib(G, N, H, W, I, O, ctypes.cast(_int_array(khs), ctypes.c_void_p),
                                          ctypes.cast(_int_array(kws), ctypes.c_void_p), dtc)


def _w6_workspace(policy, device, kib):
    """fp32 workspace of a wgrad6-reduced launch that needs ``kib`` KiB (none when kib == 0):
      "arena"  -- 2 * kib KiB of the deferred arena (the partial slabs stay there for the bank's batched reduction), else None;
      "stream" -- the per-(device, stream) cached buffer of an in-launch reduction (branches on different streams run concurrently;
                  grown outside graph capture, i.e. in the warm-up steps);
      "own"    -- the arena, else a buffer of its own outside a graph capture (the arena grows at the next step), else RuntimeError."""
    if policy == "stream":
        if kib <= 0:
            return None
        key = (device, torch.cuda.current_stream().stream_id)
        ws = _w6_ws.get(key)
        if ws is None or ws.numel() < kib * 256:
            ws = _w6_ws[key] = torch.empty(kib * 256, dtype=torch.float32, device=device)
        return ws
    ws = None
    if kib > 0:
        arena = _w6_arenas.get(device)
        if arena is None and not torch.cuda.is_current_stream_capturing():
            arena = _w6_arenas[device] = _W6Arena(device)
        ws = arena.take(2 * kib * 256) if arena is not None else None
    if ws is None and policy == "own":
        if kib > 0 and not torch.cuda.is_current_stream_capturing():
            return torch.empty(2 * kib * 256, dtype=torch.float32, device=device)
        raise RuntimeError("router trunk backward: no weight-gradient workspace (arena exhausted inside a graph capture)")
    return ws


class _ConvLayer(_collections.namedtuple("_ConvLayer", "G N H W Ho Wo Cphys I O Ipad Opad khs kws pts wstride wdstride dtc gain_val alpha beta "
                                                       "ones normalize split res_raw has_res")):
    """One stride-1 (grouped) conv layer as its launches see it: made once in _MPConvFn.forward (or from a weight-bank entry), read by the
    backward.  Cphys: stored input channels (I - 1 with the ones channel); pts: the padding of both axes; wstride / wdstride: elements per
    group of the forward / the flipped dgrad weight image; dtc: the launches' C-ABI dtype code (F32S for a split layer)."""
    __slots__ = ()

    @classmethod
    def of_entry(cls, ent, N: int, H: int, W: int, dtc: int) -> "_ConvLayer":     # a same-size bank layer over N H x W maps, no residual
        return cls(len(ent.params), N, H, W, H, W, ent.I, ent.I, ent.O, ent.Ipad, ent.Opad, ent.khs, ent.kws, [(k - 1) // 2 for k in ent.kws],
                   ent.wstride, ent.wdstride, dtc, ent.gain, ent.alpha, 0.0, False, ent.normalize, ent.dtype == "split", False, False)

    def record(self, seg, mult: float, **name) -> dict:                           # the PROFILE record of a fused launch
        return dict(**name, seg=seg, N=self.N, HW=self.H * self.W, O=self.O, I=self.Cphys, taps=[a * b for a, b in zip(self.khs, self.kws)], mult=mult)


class _BwdPlan(_collections.namedtuple("_BwdPlan", "name dtc policy mid tail defer stats label film", defaults=(False,))):
    """One fused backward launch (input + weight gradient of a weight-bank layer) as data -- _fused_bwd's arguments: entry point, dtype code,
    workspace policy (of _w6_workspace; None: no workspace), ``mid`` (or a callable that allocates the launch's own scratch, called once the
    workspace is there), ``tail``, ``defer``, ``stats``, the maker of the PROFILE record; film: hdmoe_conv_bwd6_film takes the same ``mid``."""
    __slots__ = ()

    def workspace(self, L: _ConvLayer, device) -> Optional[Tensor]:
        return _w6_workspace(self.policy, device, _w6_kib(L.G, L.N, L.H, L.W, L.Cphys, L.O, L.khs, L.kws, self.dtc))

    def launch(self, bank, ent, x, dy, dx, ws) -> bool:
        return _fused_bwd(bank, ent, self.label, self.name, x, dy, ent.wd, dx, self.mid, ws, self.tail, self.defer, self.stats)


def _kxk_bwd_plan(L: _ConvLayer, seg, policy: str, stats: tuple, kernel: str, film: bool = False, gn_in=(None, None, 0)) -> _BwdPlan:
    """hdmoe_conv_bwd6 (k x k bf16 layer: csrc/bwd6.hip, conv7_body.h) or, for L.dtc == F32S, hdmoe_conv_bwd6s (3x3 router-trunk layer: fp32
    tensors, split-bf16 arithmetic; ``gn_in`` = (scale, shift, 1): its input is relu(x * scale + shift)), both with deferred weight gradient."""
    geom, defer = (L.N, L.H, L.W, L.I, L.O, L.khs, L.kws, L.pts, L.pts, L.alpha), (seg, L.G, L.N, L.H, L.W, L.I, L.O, L.dtc, L.khs)
    if L.dtc != F32S:
        return _BwdPlan("hdmoe_conv_bwd6", L.dtc, policy, (seg, L.G, L.wdstride, *geom), (L.dtc,), defer, stats,
                        lambda: L.record(seg, 2.0, name=kernel, dtype="bfloat16"), film)
    return _BwdPlan("hdmoe_conv_bwd6s", F32S, policy, (seg, L.G, L.wdstride, L.G * L.wdstride, *geom), (*gn_in, 1 if TRUNK_BWD_BF16 else 0), defer, stats,
                    lambda: L.record(seg, 2.0, name=kernel, dtype="bfloat16" if TRUNK_BWD_BF16 else "split_bf16"))


def _conv_bwd_plan(L: _ConvLayer, seg, need_dx: bool, ones6: bool, device) -> Optional[_BwdPlan]:
    """Which fused backward launch a weight-bank layer takes, if any.  (A launch outside its own domain returns non-zero: the layer then
    takes the general path.)"""
    same = not L.ones and L.Ho == L.H and L.Wo == L.W and L.Cphys == L.I
    conv6 = need_dx and _prof_ok() and same and L.khs == L.kws
    if conv6 and L.dtc == BF16 and set(L.khs) == {3, 5}:        # 3x3 / 5x5 expert layer
        return _kxk_bwd_plan(L, seg, "arena", ("bwd6",), "bwd6_kernel", film=True)
    if conv6 and L.split and set(L.khs) == {3}:                 # a router-trunk layer run on its own
        return _kxk_bwd_plan(L, seg, "arena", ("bwd6s",), "bwd6s_kernel")
    if ones6:   # the ones-channel layer: dgrad on conv6, weight gradient on wgrad6 + pixel sums of dy (csrc/ones6.hip), reduced inside the launch
        def scratch():
            S = torch.empty((L.G, L.H, L.W, L.O), dtype=torch.float32, device=device)
            g32 = [_zeros((kh * kw, L.O, L.Cphys), torch.float32, device) for kh, kw in zip(L.khs, L.kws)]
            return (S, g32, seg, L.G, L.wdstride, L.N, L.H, L.W, L.Cphys, L.O, L.Opad, L.khs, L.alpha)
        return _BwdPlan("hdmoe_conv6_ones_bwd", L.dtc, "stream", scratch, (L.dtc,), None, (),
                        lambda: L.record(seg, 2.0 if need_dx else 1.0, name="conv6 dgrad + wgrad6 (ones-channel layer)", dtype="bfloat16"))
    if need_dx and _prof_ok() and same and L.dtc == BF16 and all(k == 1 for k in L.khs + L.kws):
        # pointwise layer (linear / 1x1): one launch that reads dy once (csrc/pbwd.hip); no workspace, the weight gradient goes straight into the bank's slabs
        return _BwdPlan("hdmoe_pw_bwd", L.dtc, None, (seg, L.G, L.wdstride, L.N, L.H * L.W, L.I, L.O, L.alpha), (L.dtc,), None, ("pbwd",),
                        lambda: L.record(seg, 2.0, name="pw_bwd_kernel", dtype="bfloat16"))
    return None


def _fused_bwd(bank, ent, label, name, x, dy, wd, dx, mid, ws, tail, defer, stats) -> bool:
    """One launch for the input gradient (into ``dx``) and the weight gradient of weight-bank layer ``ent``:
    ``name(x, dy, wd, dx, ent.G, *mid, ws, ws bytes, *tail)``.  On success ``defer`` = (seg, G, N, H, W, I, O, dtype code, khs)
    leaves the partial slabs in ``ws`` to the bank's batched reduction, the layer is noted for the bank's finish and the ``stats``
    keys are counted.  False: the layer is outside the launch's domain (nothing was launched)."""
    wsargs = () if ws is None else (ws, ws.numel() * 4)       # (ws None: a launch without workspace -- hdmoe_pw_bwd)
    if _timed("fused", label, name, x, dy, wd, dx, list(ent.G), *mid, *wsargs, *tail) != 0:
        return False
    if defer is not None:
        seg, *shape = defer
        bank.defer_w6(ent.G, seg, ws, *shape, ent=ent)
    else:
        bank.note_backward(ent)
    for k in stats:
        STATS[k] += 1
    return True


def _wgrad(x, dy, Gs, seg, G, N, H, W, Ho, Wo, I, Cphys, O, ones, khs, kws, pts, split=False, bank=None):
    """Weight gradient of a (grouped) conv into the [tap][O][I] fp32 slabs ``Gs`` (+=).  k x k bf16 layers -- and fp32 layers in
    split-bf16 mode (the router trunks) -- take the atomic-free kernel (csrc/wgrad6.hip) with a cached workspace; everything else
    the general kernel."""
    def rec(w6=None):                                         # the record of one attempt: made only when PROFILE is on and the attempt launched
        if w6:
            return lambda: _conv_record(x, seg, N, Ho * Wo, O, I, khs, kws, "split_bf16" if split else None, wgrad_name=w6)
        return lambda: _conv_record(x, seg, N, Ho * Wo, O, I, khs, kws, wgrad_name=_kernel_label(_route(
            "hdmoe_conv_wgrad_route", 34, N, H, W, Ho, Wo, I, Cphys, O, 1, ones, G, seg is not None, khs, kws, pts, pts, _dt(x),
            x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0), x, wgrad=True))
    w6 = "wgrad6_kernel<split>" if split else "wgrad6_kernel"
    if (x.dtype == torch.bfloat16 or split) and not ones and Ho == H and Wo == W and Cphys == I:
        dtc = F32S if split else _dt(x)
        kib = _w6_kib(G, N, H, W, I, O, khs, kws, dtc)
        # weight-bank layer: the partial slabs stay in the arena, the bank sums all layers' partials in one batched launch
        ws = _w6_workspace("arena", x.device, kib) if bank is not None and _prof_ok() else None
        if ws is not None:
            if _timed("conv_wgrad", rec(w6 + " (deferred reduce)"), "hdmoe_conv_wgrad6", x, dy, Gs, seg, G, N, H, W, I, O, khs, kws, pts, pts, ws, ws.numel() * 4,
                      dtc, 1) == 0:
                bank.defer_w6(Gs, seg, ws, G, N, H, W, I, O, dtc, khs)
                STATS["w6_defer"] += 1
                return
        ws = _w6_workspace("stream", x.device, kib)
        if ws is not None:
            if _timed("conv_wgrad", rec(w6 + " (+ reduce)"), "hdmoe_conv_wgrad6", x, dy, Gs, seg, G, N, H, W, I, O, khs, kws, pts, pts, ws, ws.numel() * 4, dtc, 0) == 0:
                return
    _timed("conv_wgrad", rec(), "hdmoe_conv_wgrad", x, dy, Gs, seg, G, N, H, W, Ho, Wo, I, Cphys, O, 1, 1 if ones else 0, khs, kws, pts, pts, _dt(x))


# The non-tensor argument of _MPConvFn.apply, what ops._mp_conv was asked for.  out: the output, already written by a fused launch (the
# forward then launches nothing for the conv); film: a _FilmReq -- film_silu of the output is wanted as a second output of the conv launch.
_ConvCall = _collections.namedtuple("_ConvCall", "G gain_val alpha beta ones training normalize split res_raw out film")


class _MPConvFn(torch.autograd.Function):
    """y = alpha * conv(x, prep(w)) + beta * res.   x: (N, H, W, Cphys).
    ``tensors`` = G weights followed by 0 or G learnable gain scalars (one per group)."""

    @staticmethod
    def forward(ctx, x, res, seg, c: _ConvCall, *tensors):
        G, gain_val, alpha, beta, ones, training, normalize, split = c.G, c.gain_val, c.alpha, c.beta, c.ones, c.training, c.normalize, c.split
        weights, gains = tensors[:G], list(tensors[G:]) or None
        # the input is the output of a FiLM pass (ops._FilmRec): this layer's backward may run the FiLM backward in its dgrad epilogue
        ctx.film = getattr(x, "_film_rec", None) if FILM_DGRAD and x.is_contiguous() else None
        if ctx.film is not None:
            ctx.film.register()
        x = _c(x)
        N, H, W, Cphys = x.shape
        O, I = int(weights[0].shape[0]), int(weights[0].shape[1])
        khs = [_kernel_hw(w)[0] for w in weights]
        kws = [_kernel_hw(w)[1] for w in weights]
        # reference pads by the LAST kernel dim on both axes (model_internals.py:264-270)
        pts = [(kw - 1) // 2 for kw in kws]
        Hos = {H + (kw - 1) - kh + 1 for kh, kw in zip(khs, kws)}
        if len(Hos) != 1:
            raise ValueError("grouped conv: all groups must produce the same output size")
        if any(w.shape[0] != O or w.shape[1] != I for w in weights):
            raise ValueError("grouped conv: all groups must share (out_channels, in_channels)")
        if I != Cphys + (1 if ones else 0):
            raise RuntimeError(f"MP_Conv: input has {Cphys} channels, weight expects {I}")
        Ho, Wo = Hos.pop(), W
        Ipad = (I + 15) // 16 * 16
        Opad = (O + 15) // 16 * 16
        taps = max(a * b for a, b in zip(khs, kws))
        wstride, wdstride = taps * O * Ipad, taps * I * Opad
        # split: fp32 tensors, split-bf16 arithmetic (csrc/conv6s.hip) -- weight images are bf16 [hi | lo] planes, dtype code 2
        wdt, planes, dtc = (torch.bfloat16, 2, F32S) if split else (x.dtype, 1, _dt(x))
        L = ctx.layer = _ConvLayer(G, N, H, W, Ho, Wo, Cphys, I, O, Ipad, Opad, khs, kws, pts, wstride, wdstride, dtc, gain_val, alpha, beta, ones,
                               normalize, split, c.res_raw, res is not None)
        ent = None
        if _bank.ACTIVE is not None and gains is None:
            ent = _bank.ACTIVE.lookup(weights, "split" if split else x.dtype, gain_val, alpha, normalize)
        if ent is not None:                                   # images already prepared by the bank's single launch
            wf, wd = ent.wf, ent.wd
        else:
            wf = torch.empty(planes * G * wstride, dtype=wdt, device=x.device)
            # the flipped dgrad image is produced by the same prep launch when the input needs a gradient
            wd = torch.empty(planes * G * wdstride, dtype=wdt, device=x.device) if ctx.needs_input_grad[0] else None
            call("hdmoe_wprep_fwd", list(weights), gains, gain_val, khs, kws, G, O, I, Ipad, Opad, wf, wstride, wd, wdstride,
                 1 if normalize else 0, 1 if training else 0, 1, dtc)
            if training and normalize:                         # the train-mode forward re-normalises the stored weights in place (raw pointers:
                _bank.note_weights_changed()                   #  Tensor._version stays) -- eval-mode images prepared earlier are stale
        ctx.wd, ctx.ent, ctx.bank = wd, ent, (_bank.ACTIVE if ent is not None else None)
        # the bf16 same-size bank layers without residual: the domain the two special forward launches share
        bank16 = c.out is None and ent is not None and not split and res is None and x.dtype == torch.bfloat16 and Ho == H and Wo == W
        ones_dom = bank16 and ones and ONES6 and _prof_ok() and khs == kws
        film_dom = bank16 and c.film is not None and not ones and PROFILE is None and Cphys == I
        y = c.out if c.out is not None else torch.empty((N, Ho, Wo, O), dtype=x.dtype, device=x.device)
        gb = torch.empty((G, H, W, O), dtype=torch.float32, device=x.device) if ones_dom else None
        hbuf = torch.empty_like(y) if film_dom else None
        ctx.ones6 = False
        if c.out is not None:
            pass                                              # handed in by the fused block launch (ops.unet_block_fused): nothing to launch
        elif ones_dom and _timed("fused", lambda: L.record(seg, 1.0, name="conv6_bf16_kernel (ones-channel layer)", dtype="bfloat16"),
                                 "hdmoe_conv6_ones_fwd", x, wf, y, gb, alpha, seg, G, wstride, N, H, W, Cphys, O, Ipad, khs, dtc) == 0:
            # torch.cat([x, ones]) (reference model_components.py:416): the 32 real channels on conv6, the ones channel as a bias map (csrc/ones6.hip)
            ctx.ones6 = True
            STATS["ones6"] += 1
        elif film_dom and call("hdmoe_conv_fwd_film", x, wf, y, hbuf, c.film.emb, c.film.seed, step_counter(x.device), c.film.p, alpha, seg, G, wstride,
                               N, H, W, I, O, khs, kws, pts, pts, dtc) == 0:
            # FiLM + mp_silu + dropout as a second output of this conv's epilogue (ops.mp_conv_film): one launch less on the branch's chain
            c.film.h = hbuf
        else:                                                 # (also a layer that one of the two launches above declined: nothing was launched)
            args = (x, wf, y, _c(res), alpha, beta,
                    seg, G, wstride, N, H, W, Ho, Wo, I, Cphys, Ipad, O, O, 1, 1 if ones else 0, khs, kws, pts, pts, dtc)
            _timed("conv_fwd", lambda: _fwd_record(*args), "hdmoe_conv_fwd", *args)
        ctx.save_for_backward(x, seg, *tensors)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, seg, *tensors = ctx.saved_tensors
        L, nig = ctx.layer, ctx.needs_input_grad
        weights, gains = tensors[:L.G], list(tensors[L.G:]) or None
        dy = _c(dy)
        need_gain = gains is not None and any(nig[4 + L.G:])
        need_w = any(nig[4:4 + L.G]) or need_gain
        fused, dx = _conv_fused_bwd(ctx, L, x, dy, seg, nig[0]) if need_w and ctx.ent is not None else (False, None)
        if nig[0] and not fused:
            dx = _conv_dgrad(L, x, dy, ctx.wd, seg)
        dres = None
        if L.has_res and nig[1]:
            if L.res_raw or L.beta == 1.0:
                dres = dy                                     # beta == 1, or the producer of `res` applies beta in its own backward pass
            else:
                dres = torch.empty_like(dy)
                call("hdmoe_axpby", dres, dy, None, L.beta, 0.0, dy.numel(), _dt(dy))
        dws, dgs = _conv_wgrad(ctx, L, x, dy, seg, weights, gains, need_gain) if need_w and not fused else ([None] * L.G, [None] * len(gains or ()))
        return (dx, dres, None, None, *dws, *dgs)


def _conv_fused_bwd(ctx, L: _ConvLayer, x, dy, seg, need_dx: bool):
    """The fused step of a weight-bank layer's backward -> (launched?, dx): input and weight gradient in one launch (ops._conv_bwd_plan); behind
    a FiLM pass (ctx.film) first the launch that also runs the FiLM backward, in its dgrad epilogue."""
    rec = ctx.film
    if rec is not None:
        rec.clear()
    plan = _conv_bwd_plan(L, seg, need_dx, ctx.ones6, x.device)
    ws = plan.workspace(L, x.device) if plan is not None and plan.policy is not None else None
    if plan is None or (ws is None and plan.policy is not None):
        return False, None
    if callable(plan.mid):
        plan = plan._replace(mid=plan.mid())
    dx = torch.empty_like(x) if need_dx else None
    fused = False
    if plan.film and rec is not None and FILM_DGRAD and need_dx and rec.sole_consumer(x):
        # dx of this launch is then du of the FiLM pass, de its embedding gradient (csrc/conv7_body.h, EPI = 1); outside the
        # epilogue's domain the entry returns non-zero without launching and the layer takes the plain launch below
        de = torch.empty(rec.e.shape, dtype=torch.float32, device=x.device)
        fused = plan._replace(name="hdmoe_conv_bwd6_film", tail=(rec.u, rec.e, rec.mask, de, rec.p, plan.dtc),
                              label=lambda: dict(plan.label(), name="bwd7_kernel (FiLM epilogue)")).launch(ctx.bank, ctx.ent, x, dy, dx, ws)
        if fused:
            rec.offer(dx, de)
            STATS["film_dgrad"] += 1
    fused = fused or plan.launch(ctx.bank, ctx.ent, x, dy, dx, ws)
    return fused, dx if fused else None


def _conv_dgrad(L: _ConvLayer, x, dy, wd, seg) -> Tensor:
    """The input gradient on its own: conv over dy (O channels) with the flipped kernel; logical out channels I, stored Cphys."""
    dx = torch.empty_like(x)
    pt_d = [kh - 1 - p for kh, p in zip(L.khs, L.pts)]
    pl_d = [kw - 1 - p for kw, p in zip(L.kws, L.pts)]
    args = (dy, wd, dx, None, L.alpha, 0.0,
            seg, L.G, L.wdstride, L.N, L.Ho, L.Wo, L.H, L.W, L.O, L.O, L.Opad, L.I, L.Cphys, 1, 0, L.khs, L.kws, pt_d, pl_d, L.dtc)
    _timed("conv_fwd", lambda: _fwd_record(*args), "hdmoe_conv_fwd", *args)
    return dx


def _conv_wgrad(ctx, L: _ConvLayer, x, dy, seg, weights, gains, need_gain: bool):
    """The weight gradient on its own -> (dws, dgs) for autograd.  A weight-bank layer accumulates into the bank's slabs (one multi-tensor
    launch at the end of backward finishes every gradient) and hands autograd None."""
    G, O, I = L.G, L.O, L.I
    geom = (seg, G, L.N, L.H, L.W, L.Ho, L.Wo, I, L.Cphys, O, L.ones, L.khs, L.kws, L.pts, L.split)
    dgs = [None] * len(gains or ())
    if ctx.ent is not None:
        _wgrad(x, dy, ctx.ent.G, *geom, bank=ctx.bank)
        ctx.bank.note_backward(ctx.ent)
        return [None] * G, dgs
    sizes = [kh * kw * O * I for kh, kw in zip(L.khs, L.kws)]
    Gs = list(torch.zeros(sum(sizes), dtype=torch.float32, device=x.device).split(sizes))       # one memset for all groups
    _wgrad(x, dy, Gs, *geom)
    dws = [torch.empty_like(w) for w in weights]
    if need_gain:
        dgs = [torch.zeros((), dtype=torch.float32, device=x.device) for _ in range(G)]
    call("hdmoe_wprep_bwd", list(weights), gains, L.gain_val, Gs, dws, dgs if need_gain else None, L.khs, L.kws, G, O, I, 1 if L.normalize else 0)
    if L.alpha != 1.0:
        for d in dws + [d for d in dgs if d is not None]:
            call("hdmoe_axpby", d, d, None, L.alpha, 0.0, d.numel(), 0)
    return dws, dgs



class _StridedConvFn(torch.autograd.Function):
    """MP_Conv with stride > 1 (reference model_internals.py:272-275: F.conv2d(x, w, padding=k // 2, stride)).  No reference model uses
    it; forward and weight gradient run on the general strided kernels (the patch embedding's), the input gradient is not implemented."""

    @staticmethod
    def forward(ctx, x, w, gain, stride, training):
        x = _c(x)
        N, H, W, C = x.shape
        O, I, kh, kw = (int(v) for v in w.shape)
        if I != C:
            raise RuntimeError(f"MP_Conv: input has {C} channels, weight expects {I}")
        pad = kw // 2                                          # the reference pads both axes by the last kernel dim
        Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        Ipad = (I + 15) // 16 * 16
        wf = torch.empty(kh * kw * O * Ipad, dtype=x.dtype, device=x.device)
        call("hdmoe_wprep_fwd", [w], None, float(gain), [kh], [kw], 1, O, I, Ipad, 16, wf, wf.numel(), None, 0, 1, 1 if training else 0, 1, _dt(x))
        if training:
            _bank.note_weights_changed()
        y = torch.empty((N, Ho, Wo, O), dtype=x.dtype, device=x.device)
        call("hdmoe_conv_fwd", x, wf, y, None, 1.0, 0.0, None, 1, wf.numel(), N, H, W, Ho, Wo, I, I, Ipad, O, O, stride, 0, [kh], [kw], [pad], [pad], _dt(x))
        ctx.save_for_backward(x, w)
        ctx.meta = (float(gain), stride, pad, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        gain, stride, pad, Ho, Wo = ctx.meta
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("MP_Conv(stride > 1): the input gradient is not implemented (no reference model uses a strided MP_Conv)")
        N, H, W, C = x.shape
        O, I, kh, kw = (int(v) for v in w.shape)
        dw = None
        if ctx.needs_input_grad[1]:
            Gs = [_zeros((kh * kw, O, I), torch.float32, x.device)]
            call("hdmoe_conv_wgrad", x, _c(dy), Gs, None, 1, N, H, W, Ho, Wo, I, I, O, stride, 0, [kh], [kw], [pad], [pad], _dt(x))
            dw = torch.empty_like(w)
            call("hdmoe_wprep_bwd", [w], None, gain, Gs, [dw], None, [kh], [kw], 1, O, I, 1)
        return None, dw, None, None, None


def mp_conv_strided(x: Tensor, w: Tensor, gain: float, stride: int, training: bool = False) -> Tensor:
    (w,) = f32_params([w])
    return _StridedConvFn.apply(x, w, float(gain), int(stride), bool(training))


def _split_ok(N: int, H: int, W: int, C: int, ws) -> bool:
    """Does the split-bf16 conv kernel (csrc/conv6s.hip) take the layer -- fp32 (N, H, W, C) input, weights ``ws``?  The library says (the
    route of an HDMOE_F32S call); asked ahead of the launch because the weight image format depends on the answer."""
    if any(w.ndim != 4 for w in ws):
        return False
    O, khs, kws = int(ws[0].shape[0]), [int(w.shape[2]) for w in ws], [int(w.shape[3]) for w in ws]
    pts = [(k - 1) // 2 for k in kws]
    return _route("hdmoe_conv_fwd_route", 5, N, H, W, H, W, C, C, (C + 15) // 16 * 16, O, O, 1, 0, len(ws), len(ws) > 1, 0,
                  max(a * b for a, b in zip(khs, kws)) * O * ((C + 15) // 16 * 16), khs, kws, pts, pts, F32S, 1)[0] == ROUTE_CONV6S


def mp_conv(x: Tensor, weights, gain=1.0, *, seg: Optional[Tensor] = None, res: Optional[Tensor] = None, alpha: float = 1.0,
            beta: float = 0.0, ones: bool = False, training: bool = False, normalize: bool = True, split: bool = False,
            res_grad_raw: bool = False) -> Tensor:
    """Magnitude-preserving conv / linear (reference MP_Conv.forward, model_internals.py:253-275).

    ``x``: (N,H,W,C) -> (N,Ho,Wo,O);  (N,S,C) -> (N,S,O);  (M,C) -> (M,O).  ``weights``: a tensor, or a list of
    per-expert tensors together with ``seg`` (device int32 row offsets) for a grouped launch.
    ``gain``: python float, a 0-dim float32 tensor (learnable out_gain), or a list of such tensors (one per group)."""
    return _mp_conv(x, weights, gain, seg=seg, res=res, alpha=alpha, beta=beta, ones=ones, training=training, normalize=normalize, split=split,
                    res_grad_raw=res_grad_raw)


def _mp_conv(x, weights, gain=1.0, *, seg=None, res=None, alpha=1.0, beta=0.0, ones=False, training=False, normalize=True, split=False,
             res_grad_raw=False, out: Optional[Tensor] = None, film: Optional["_FilmReq"] = None) -> Tensor:
    """ops.mp_conv, and how a fused launch hands its outputs to the unfused autograd graph: ``out`` is the (N, Ho, Wo, O) output a fused
    launch has already written -- the forward launches nothing for the conv, the graph node and the saved tensors are as usual
    (ops.unet_block_fused); ``film`` asks for film_silu of the output as a second output of the conv launch and receives it (ops.mp_conv_film)."""
    ws = f32_params(list(weights) if isinstance(weights, (list, tuple)) else [weights])
    G = len(ws)
    if isinstance(gain, (list, tuple)):
        gts, gain_val = f32_params(list(gain)), 1.0
    elif torch.is_tensor(gain):
        gts, gain_val = f32_params([gain]) * G, 1.0
    else:
        gts, gain_val = [], float(gain)
    shape = x.shape
    grouped = seg is not None
    if x.ndim not in (2, 3, 4):
        raise ValueError("mp_conv: x must be 2-, 3- or 4-D")
    pointwise = all(w.ndim == 2 or (w.shape[2] == 1 and w.shape[3] == 1) for w in ws)
    if pointwise and not grouped and not ones:
        # 1x1 / linear layer without per-row experts: every position is independent, so present the tensor as ONE long row
        # of positions -- tiles are then always full (a (B,16,C) token tensor would otherwise fill 16 of 128 tile slots)
        x4 = x.reshape(1, 1, -1, shape[-1])
    elif x.ndim == 2:
        x4 = x.reshape(shape[0], 1, 1, shape[1])
    elif x.ndim == 3:
        x4 = x.reshape(shape[0], 1, shape[1], shape[2])
    else:
        x4 = x
    if res is not None:
        res = res.reshape(x4.shape[0], x4.shape[1], x4.shape[2], -1)
    split = bool(split) and not ones and x4.dtype == torch.float32 and _split_ok(*x4.shape, ws)
    # res_grad_raw: the gradient handed back for `res` is dy itself, NOT beta * dy -- only for a `res` whose producer was created with
    # gx_scale = beta (ops.silu_branch / ops.pixel_norm_silu) and has no other consumer: saves a scaling pass per residual block
    c = _ConvCall(G, gain_val, float(alpha), float(beta), bool(ones), bool(training), bool(normalize), split, bool(res_grad_raw), out, film)
    y = _MPConvFn.apply(x4, res, seg, c, *ws, *gts)
    return y.reshape(*shape[:-1], y.shape[-1])


class _MultiLinearFn(torch.autograd.Function):
    """L linear layers over the same fp32 input in one launch each for forward / input gradient / weight gradient
    (csrc/mlinear.hip).  ``tensors`` = L * G weights (layer-major); every layer must be a ready weight-bank entry."""

    @staticmethod
    def forward(ctx, x, seg, ents, bank, c, *tensors):
        x = _f32(x)
        R, I = x.shape
        L = len(ents)
        G = len(ents[0].params)
        Os = [e.O for e in ents]
        ys = [torch.empty((R, o), dtype=torch.float32, device=x.device) for o in Os]
        call("hdmoe_mlinear_fwd", ys, x, [e.wf for e in ents], seg, Os, L, R, I, ents[0].Ipad, G, c)
        ctx.save_for_backward(x, seg)
        ctx.meta = (ents, bank, Os, G)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gs):
        x, seg = ctx.saved_tensors
        ents, bank, Os, G = ctx.meta
        R, I = x.shape
        L = len(ents)
        gs = [_f32(g) if g is not None else _zeros((R, o), torch.float32, x.device) for g, o in zip(gs, Os)]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            call("hdmoe_mlinear_dgrad", dx, gs, [e.wf for e in ents], seg, Os, L, R, I, ents[0].Ipad, G)
        if any(ctx.needs_input_grad[5:]):
            Gs = []
            for e in ents:
                Gs += list(e.G) + [None] * (8 - G)
            call("hdmoe_mlinear_wgrad", Gs, gs, x, seg, Os, L, R, I, G)
            for e in ents:
                bank.note_backward(e)
        return (dx, None, None, None, None) + (None,) * (L * G)


def multi_linear(x: Tensor, layers, gain: float, *, seg: Optional[Tensor] = None, c: float = 0.0, training: bool = False):
    """[c + mp_linear_l(x) for l in layers] for MP_Conv layers (kernel ()) that all read ``x`` (R, I) fp32; ``layers`` = list of per-layer
    weight lists (one weight per expert with ``seg``).  One launch for all layers once the weight bank has their images; the plain
    per-layer path otherwise (first steps, no bank, more than 16 layers)."""
    L = len(layers)
    bank = _bank.ACTIVE
    ents = None
    if bank is not None and 1 <= L <= 16 and x.ndim == 2 and x.shape[1] <= 256 and x.dtype == torch.float32:
        ents = [bank.lookup(ws, torch.float32, float(gain), 1.0, True) for ws in layers]
        ok = all(e is not None for e in ents) and len({(e.I, e.Ipad, len(e.params)) for e in ents if e is not None}) == 1
        if ok and all(e.khs == [1] * len(e.params) for e in ents) and (seg is not None or len(ents[0].params) == 1):
            flat = [w for ws in layers for w in ws]
            return list(_MultiLinearFn.apply(x, seg, ents, bank, float(c), *flat))
    outs = [mp_conv(x, ws if seg is not None else ws[0], gain, seg=seg, training=training) for ws in layers]
    return [affine(o, 1.0, c) for o in outs] if c != 0.0 else outs



def _call_or(fast: str, plain: str, *args) -> None:
    """Run the entry point `fast`; where it declines the shape (return code 1: nothing launched), run `plain`, the kernel it replaces."""
    if call(fast, *args) == 1:
        call(plain, *args)


class _PatchLinearFn(torch.autograd.Function):
    """Vit_expert.patch when the image divides into patches (model_components.py:670-679): a stride-p p x p conv is a linear layer on
    the patch vectors, so: one relayout pass (image -> tokens of C*p*p features in the weight's own (c, i, j) order, the parameter
    is used as the [E][C*p*p] matrix it already is in memory), then the long-contraction pointwise kernel (csrc/kgemm.hip), and in
    the backward the streamed pointwise weight gradient (csrc/lwgrad.hip) -- instead of the generic strided conv kernels, whose
    weight gradient alone cost 190 us per expert."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = _c(x)
        N, H, W, C = x.shape
        E, p = int(w.shape[0]), int(w.shape[2])
        hp, wp, K = H // p, W // p, C * p * p
        Epad = (E + 15) // 16 * 16
        tok = torch.empty((N, hp, wp, K), dtype=x.dtype, device=x.device)
        _call_or("hdmoe_patch_relayout_tiled", "hdmoe_patch_relayout", tok, x, N, H, W, C, p, hp, wp, 1, 0, _dt(x))
        wf = torch.empty(E * K, dtype=x.dtype, device=x.device)
        wd = torch.empty(K * Epad, dtype=x.dtype, device=x.device) if ctx.needs_input_grad[0] else None
        call("hdmoe_wprep_fwd", [w], None, 1.0, [1], [1], 1, E, K, K, Epad, wf, wf.numel(), wd, 0 if wd is None else wd.numel(), 0, 0, 0, _dt(x))
        y0 = torch.empty((N, hp, wp, E), dtype=x.dtype, device=x.device)
        call("hdmoe_conv_fwd", tok, wf, y0, None, 1.0, 0.0, None, 1, wf.numel(), N, hp, wp, hp, wp, K, K, K, E, E, 1, 0, [1], [1], [0], [0], _dt(x))
        y = torch.empty_like(y0)
        call("hdmoe_bias_add", y, y0, b, N * hp * wp, E, _dt(x))
        ctx.save_for_backward(tok, w)
        ctx.wd = wd
        ctx.dims = (N, H, W, C, E, p, hp, wp, K, Epad)
        return y.reshape(N, hp * wp, E)

    @staticmethod
    def backward(ctx, dy):
        tok, w = ctx.saved_tensors
        N, H, W, C, E, p, hp, wp, K, Epad = ctx.dims
        dy = _c(dy).reshape(N, hp, wp, E)
        dt = _dt(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dtok = torch.empty((N, hp, wp, K), dtype=dy.dtype, device=dy.device)
            call("hdmoe_conv_fwd", dy, ctx.wd, dtok, None, 1.0, 0.0, None, 1, ctx.wd.numel(), N, hp, wp, hp, wp, E, E, Epad, K, K, 1, 0, [1], [1], [0], [0], dt)
            dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
            _call_or("hdmoe_patch_relayout_tiled", "hdmoe_patch_relayout", dx, dtok, N, H, W, C, p, hp, wp, 1, 1, dt)
        if ctx.needs_input_grad[1]:
            Gs = [_zeros((1, E, K), torch.float32, dy.device)]
            call("hdmoe_conv_wgrad", tok, dy, Gs, None, 1, N, hp, wp, hp, wp, K, K, E, 1, 0, [1], [1], [0], [0], dt)
            dw = torch.empty_like(w)
            call("hdmoe_wprep_bwd", [w], None, 1.0, Gs, [dw], None, [1], [1], 1, E, K, 0)
        if ctx.needs_input_grad[2]:
            db = torch.zeros(E, dtype=torch.float32, device=dy.device)
            call("hdmoe_colsum", db, dy, N * hp * wp, E, dt)
        return dx, dw, db


class _PatchEmbedFn(torch.autograd.Function):
    """Vit_expert.patch: nn.Conv2d(C, E, p, stride=p) with bias on the zero-padded image (model_components.py:670-679)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = _c(x)
        N, H, W, C = x.shape
        E, p = int(w.shape[0]), int(w.shape[2])
        hp, wp = -(-H // p), -(-W // p)
        Ipad = (C + 15) // 16 * 16
        wf = torch.empty(p * p * E * Ipad, dtype=x.dtype, device=x.device)
        call("hdmoe_wprep_fwd", [w], None, 1.0, [p], [p], 1, E, C, Ipad, 16, wf, wf.numel(), None, 0, 0, 0, 0, _dt(x))
        y0 = torch.empty((N, hp, wp, E), dtype=x.dtype, device=x.device)
        call("hdmoe_conv_fwd", x, wf, y0, None, 1.0, 0.0, None, 1, wf.numel(), N, H, W, hp, wp, C, C, Ipad, E, E, p, 0, [p], [p],
             [0], [0], _dt(x))
        y = torch.empty_like(y0)
        call("hdmoe_bias_add", y, y0, b, N * hp * wp, E, _dt(x))
        ctx.save_for_backward(x, w)
        return y.reshape(N, hp * wp, E)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, H, W, C = x.shape
        E, p = int(w.shape[0]), int(w.shape[2])
        hp, wp = -(-H // p), -(-W // p)
        dy = _c(dy).reshape(N, hp, wp, E)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            Ipad = (C + 15) // 16 * 16
            Epad = (E + 15) // 16 * 16
            wf = torch.empty(p * p * E * Ipad, dtype=x.dtype, device=x.device)
            wd = torch.empty(p * p * C * Epad, dtype=x.dtype, device=x.device)     # [(tap, c)][Epad] == 1x1 weight, p*p*C outputs
            call("hdmoe_wprep_fwd", [w], None, 1.0, [p], [p], 1, E, C, Ipad, Epad, wf, wf.numel(), wd, wd.numel(), 0, 0, 0, _dt(x))
            tok = torch.empty((N, hp, wp, p * p * C), dtype=x.dtype, device=x.device)
            call("hdmoe_conv_fwd", dy, wd, tok, None, 1.0, 0.0, None, 1, wd.numel(), N, hp, wp, hp, wp, E, E, Epad, p * p * C,
                 p * p * C, 1, 0, [1], [1], [0], [0], _dt(x))
            dx = torch.empty_like(x)
            call("hdmoe_patch_relayout", dx, tok, N, H, W, C, p, hp, wp, 0, 1, _dt(x))
        if ctx.needs_input_grad[1]:
            Gs = [_zeros((p * p, E, C), torch.float32, x.device)]
            call("hdmoe_conv_wgrad", x, dy, Gs, None, 1, N, H, W, hp, wp, C, C, E, p, 0, [p], [p], [0], [0], _dt(x))
            dw = torch.empty_like(w)
            call("hdmoe_wprep_bwd", [w], None, 1.0, Gs, [dw], None, [p], [p], 1, E, C, 0)
        if ctx.needs_input_grad[2]:
            db = torch.zeros(E, dtype=torch.float32, device=x.device)
            call("hdmoe_colsum", db, dy, N * hp * wp, E, _dt(x))
        return dx, dw, db


def patch_embed(x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    """(N,H,W,C) -> tokens (N, ceil(H/p)*ceil(W/p), E)."""
    p = int(w.shape[2])
    if (x.shape[1] % p == 0 and x.shape[2] % p == 0 and w.shape[2] == w.shape[3] and w.is_contiguous()
            and x.shape[3] % (8 if x.dtype == torch.bfloat16 else 4) == 0 and (x.shape[3] * p * p) % 16 == 0):
        return _PatchLinearFn.apply(x, w, b)
    return _PatchEmbedFn.apply(x, w, b)


# =====================================================================================================
# pointwise
# =====================================================================================================
class _AxpbyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, a, b):
        x = _c(x); y = _c(y)
        out = torch.empty_like(x)
        call("hdmoe_axpby", out, x, y, a, b, x.numel(), _dt(x))
        ctx.ab = (a, b, y is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, has_y = ctx.ab
        g = _c(g)
        dx = dy = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(g); call("hdmoe_axpby", dx, g, None, a, 0.0, g.numel(), _dt(g))
        if has_y and ctx.needs_input_grad[1]:
            if dx is not None and a == b:
                dy = dx                                       # equal weights (mp_sum with t = 0.5): one scaled copy serves both inputs
            else:
                dy = torch.empty_like(g); call("hdmoe_axpby", dy, g, None, b, 0.0, g.numel(), _dt(g))
        return dx, dy, None, None


def axpby(x: Tensor, y: Optional[Tensor], a: float, b: float = 0.0) -> Tensor:
    return _AxpbyFn.apply(x, y, float(a), float(b))


# ---- EDM sampler stage (fp32 latents, schedule t and stage index idx on the device; see include/hdmoe.h).  `known` = (x0, noise, mask) of
# the inpainting blend epilogue, or None.  Written into preallocated buffers so that the calls can be captured.
# Stochastic stages: `seed` = device int64 word holding the call's 64-bit seed, `t_hat` = device float64 word (the churned sigma); stage i
# draws the values of randn_keyed(.., seed, i).
def heun_euler(xn: Tensor, xh: Tensor, den: Tensor, t: Tensor, idx: Tensor, known: Optional[Sequence[Tensor]] = None,
               t_hat: Optional[Tensor] = None) -> None:
    x0, nz, m = known if known is not None else (None, None, None)
    if t_hat is None:
        call("hdmoe_heun_euler", xn, xh, den, t, idx, xn.numel(), x0, nz, m)
    else:
        call("hdmoe_heun_euler_hat", xn, xh, den, t, idx, t_hat, xn.numel(), x0, nz, m)


def heun_correct(out: Tensor, xh: Tensor, den: Tensor, xn: Tensor, den2: Tensor, t: Tensor, idx: Tensor,
                 known: Optional[Sequence[Tensor]] = None, t_hat: Optional[Tensor] = None) -> None:
    x0, nz, m = known if known is not None else (None, None, None)
    if t_hat is None:
        call("hdmoe_heun_correct", out, xh, den, xn, den2, t, idx, out.numel(), x0, nz, m)
    else:
        call("hdmoe_heun_correct_hat", out, xh, den, xn, den2, t, idx, t_hat, out.numel(), x0, nz, m)


def heun_churn(x_hat: Tensor, x: Tensor, sigma: Tensor, t_hat: Tensor, t: Tensor, idx: Tensor, seed: Tensor, gamma_cap: float, s_min: float,
               s_max: float, s_noise: float) -> None:
    """Churn of Heun stage i = idx: t_hat = t[i] (1 + gamma) into t_hat (float64) and sigma (float32), x_hat = x + sqrt(t_hat^2 - t[i]^2)
    s_noise eps (x_hat may be x).  gamma = gamma_cap where s_min <= t[i] <= s_max, else 0 (then x_hat = x and nothing is drawn)."""
    call("hdmoe_heun_churn", x_hat, x, sigma, t_hat, t, idx, seed, float(gamma_cap), float(s_min), float(s_max), float(s_noise), x_hat.numel())


def dpm2m_sde_step(out: Tensor, x: Tensor, den: Tensor, den_prev: Tensor, t: Tensor, idx: Tensor, i0: Tensor, eta: float, s_noise: float,
                   seed: Tensor, known: Optional[Sequence[Tensor]] = None) -> None:
    """One DPM-Solver++(2M) SDE stage (midpoint form) into out: dpm2m_step with the decay exp(-eta h) on x and the stage's noise added."""
    x0, nz, m = known if known is not None else (None, None, None)
    call("hdmoe_dpm2m_sde_step", out, x, den, den_prev, t, idx, i0, out.numel(), x0, nz, m, float(eta), float(s_noise), seed)


def dpm2m_step(out: Tensor, x: Tensor, den: Tensor, den_prev: Tensor, t: Tensor, idx: Tensor, i0: Tensor,
               known: Optional[Sequence[Tensor]] = None) -> None:
    """One DPM-Solver++(2M) stage into out (out may be x); reads den_prev, then stores den into it.  i0 = device int32 first stage."""
    x0, nz, m = known if known is not None else (None, None, None)
    call("hdmoe_dpm2m_step", out, x, den, den_prev, t, idx, i0, out.numel(), x0, nz, m)


def known_blend_(x: Tensor, x0: Tensor, noise: Tensor, mask: Tensor, s: float) -> Tensor:
    """In place: x <- mask (x0 + s noise) + (1 - mask) x; x, x0, noise contiguous of one dtype, mask fp32, all of x's size."""
    assert x.is_contiguous() and x0.is_contiguous() and noise.is_contiguous() and mask.is_contiguous()
    assert x0.dtype == noise.dtype == x.dtype and mask.dtype == torch.float32 and x0.numel() == noise.numel() == mask.numel() == x.numel()
    call("hdmoe_known_blend", x, x0, noise, mask, float(s), x.numel(), _dt(x))
    return x


# ---- tiled sampling: a latent larger than the model's resolution is evaluated on overlapping model-sized windows (MultiDiffusion) --------
TILE_MAX_AXIS = 32                        # HDMOE_TILE_MAX_AXIS of include/hdmoe.h: tiles along one axis
TILE_WINDOWS = ("uniform", "feather")


class TilePlan:
    """Where the (h, w) windows of an (H, W) latent lie and how their outputs blend; built by tile_plan() on the host (numpy only).
      oy (Ty,), ox (Tx,)       int32 origins along y / x
      ny (Ty, H), nx (Tx, W)   float32 normalised 1-D window weights: ny[k, y] = w1(y - oy[k]) / sum_k' w1(y - oy[k']) where tile k covers
                               row y, 0 elsewhere (computed in float64, rounded once).  The 2-D weight of tile (ky, kx) is ny[ky, y] nx[kx, x].
      Ty, Tx, T = Ty Tx        tile counts;  max_cover_y / max_cover_x / max_cover = their product: the most tiles over one position
    Tile-batch row order is sample-major: r = (b Ty + ky) Tx + kx.  device(dev): the four arrays as tensors on dev (made once per device;
    ask for them before a stream capture)."""

    def __init__(self, H, W, h, w, overlap, window, oy, ox, ny, nx):
        self.H, self.W, self.h, self.w, self.overlap, self.window = H, W, h, w, overlap, window
        self.oy, self.ox, self.ny, self.nx = oy, ox, ny, nx
        self.Ty, self.Tx = int(oy.shape[0]), int(ox.shape[0])
        self.T = self.Ty * self.Tx
        self.max_cover_y = int((ny > 0).sum(0).max())
        self.max_cover_x = int((nx > 0).sum(0).max())
        self.max_cover = self.max_cover_y * self.max_cover_x
        self._dev = {}

    def device(self, dev):
        dev = torch.device(dev)
        if dev not in self._dev:
            self._dev[dev] = tuple(torch.from_numpy(a).to(dev) for a in (self.oy, self.ox, self.ny, self.nx))
        return self._dev[dev]

    def __repr__(self):
        return (f"TilePlan({self.H}x{self.W} in {self.Ty}x{self.Tx} tiles of {self.h}x{self.w}, overlap={self.overlap}, "
                f"window={self.window!r}, max_cover={self.max_cover})")


def _tile_axis(L: int, n: int, o: int, window: str, axis: str):
    """Origins (int32) and the normalised weight table (T, L) float32 of one axis: stride s = n - o, 1 + ceil((L - n) / s) tiles, origin k
    = min(k s, L - n) (the last tile is clamped to the edge)."""
    import numpy as np
    if L < n:
        raise ValueError(f"tile_plan: the latent's {axis} ({L}) is smaller than the tile's ({n})")
    if not 0 <= o < n:
        raise ValueError(f"tile_plan: overlap along {axis} must lie in [0, {n}), got {o}")
    s = n - o
    T = 1 if L == n else 1 + -(-(L - n) // s)
    if T > TILE_MAX_AXIS:
        raise ValueError(f"tile_plan: {T} tiles along {axis} ({L} in tiles of {n}, overlap {o}); the limit is {TILE_MAX_AXIS}")
    org = np.minimum(np.arange(T, dtype=np.int64) * s, L - n)
    i = np.arange(L, dtype=np.int64)[None, :] - org[:, None]                  # tile-local index of every position, (T, L)
    inside = (i >= 0) & (i < n)
    if window == "uniform":
        w1 = np.ones(i.shape, dtype=np.float64)
    else:
        r = max(o, 1)
        w1 = np.minimum(np.minimum(i + 1, n - i), r).astype(np.float64) / r
    w1 = np.where(inside, w1, 0.0)
    return org.astype(np.int32), (w1 / w1.sum(0, keepdims=True)).astype(np.float32)


def tile_plan(H: int, W: int, h: int, w: int, overlap=0, window: str = "feather") -> TilePlan:
    """The plan of (h, w) tiles over an (H, W) latent.  overlap: an int or (oy, ox), 0 <= overlap < tile; window: "uniform" (w1 = 1) or
    "feather" (w1(i) = min(i + 1, n - i, r) / r, r = max(overlap, 1)).  ValueError: a latent smaller than the tile, an overlap outside
    [0, n), more than 32 tiles on an axis, an unknown window.  Pure host arithmetic."""
    if window not in TILE_WINDOWS:
        raise ValueError(f"tile_plan: window must be one of {', '.join(map(repr, TILE_WINDOWS))}, got {window!r}")
    try:
        ov = (int(overlap),) * 2 if isinstance(overlap, numbers.Integral) else tuple(int(v) for v in overlap)
        dims = tuple(int(v) for v in (H, W, h, w))
    except (TypeError, ValueError):
        raise ValueError(f"tile_plan: sizes must be ints and overlap an int or a pair (oy, ox), got {(H, W, h, w)!r}, {overlap!r}") from None
    if len(ov) != 2 or min(dims) < 1:
        raise ValueError(f"tile_plan: sizes must be positive and overlap an int or a pair (oy, ox), got {(H, W, h, w)!r}, {overlap!r}")
    H, W, h, w = dims
    oy, ny = _tile_axis(H, h, ov[0], window, "H")
    ox, nx = _tile_axis(W, w, ov[1], window, "W")
    return TilePlan(H, W, h, w, ov, window, oy, ox, ny, nx)


def _tile_check(who: str, t: Tensor, shape, what: str) -> Tensor:
    if not isinstance(t, Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{who}: {what} must be a contiguous float32 CUDA tensor of shape {tuple(shape)}, got "
                         f"{tuple(getattr(t, 'shape', ())) or type(t).__name__} {getattr(t, 'dtype', '')}")
    return t.detach()


def tile_gather(x: Tensor, plan: TilePlan, row0: int = 0, rows: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """Rows row0 .. row0 + rows - 1 (default: all B T) of the tile batch of x (B, C, H, W), float32: (rows, C, h, w), an exact copy of the
    windows in the plan's sample-major order.  out: a preallocated result (a captured launch).  Inference only."""
    if not isinstance(x, Tensor) or x.ndim != 4 or tuple(x.shape[2:]) != (plan.H, plan.W):
        raise ValueError(f"tile_gather: x must be (B, C, {plan.H}, {plan.W}), got {tuple(getattr(x, 'shape', ())) or type(x).__name__}")
    x = _tile_check("tile_gather", x, x.shape, "x")
    B, C = int(x.shape[0]), int(x.shape[1])
    total = B * plan.T
    rows = total - int(row0) if rows is None else int(rows)
    row0 = int(row0)
    if row0 < 0 or rows < 1 or row0 + rows > total:
        raise ValueError(f"tile_gather: rows [{row0}, {row0 + rows}) do not lie in the tile batch of {total} rows")
    shape = (rows, C, plan.h, plan.w)
    out = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else _tile_check("tile_gather", out, shape, "out")
    oy, ox, _, _ = plan.device(x.device)
    call("hdmoe_tile_gather", out, x, oy, ox, B, C, plan.H, plan.W, plan.h, plan.w, plan.Ty, plan.Tx, row0, rows)
    return out


def tile_blend(tiles: Tensor, plan: TilePlan, B: int, out: Optional[Tensor] = None) -> Tensor:
    """The (B, C, H, W) blend of the tile batch tiles (B T, C, h, w), float32:
    out[b, c, y, x] = sum_ky sum_kx (ny[ky, y] nx[kx, x]) tiles[(b Ty + ky) Tx + kx, c, y - oy[ky], x - ox[kx]] over the covering tiles,
    fp32 fma in that order, every element written once (deterministic).  out: a preallocated result.  Inference only."""
    B = int(B)
    if not isinstance(tiles, Tensor) or tiles.ndim != 4 or B < 1 or tuple(tiles.shape) != (B * plan.T, tiles.shape[1], plan.h, plan.w):
        raise ValueError(f"tile_blend: tiles must be (B T = {B * plan.T}, C, {plan.h}, {plan.w}), got "
                         f"{tuple(getattr(tiles, 'shape', ())) or type(tiles).__name__}")
    tiles = _tile_check("tile_blend", tiles, tiles.shape, "tiles")
    C = int(tiles.shape[1])
    shape = (B, C, plan.H, plan.W)
    out = torch.empty(shape, dtype=torch.float32, device=tiles.device) if out is None else _tile_check("tile_blend", out, shape, "out")
    oy, ox, ny, nx = plan.device(tiles.device)
    call("hdmoe_tile_blend", out, tiles, oy, ox, ny, nx, B, C, plan.H, plan.W, plan.h, plan.w, plan.Ty, plan.Tx)
    return out


def mp_sum(a: Tensor, b: Tensor, t: float = 0.5) -> Tensor:
    """lerp(a,b,t)/sqrt((1-t)^2+t^2) (model_internals.py:50-66)."""
    n = math.sqrt((1.0 - t) ** 2 + t ** 2)
    return axpby(a, b, (1.0 - t) / n, t / n)


class _AffineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, c):
        x = _c(x)
        out = torch.empty_like(x)
        call("hdmoe_affine", out, x, a, c, x.numel(), _dt(x))
        ctx.a = a
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        dx = torch.empty_like(g)
        call("hdmoe_axpby", dx, g, None, ctx.a, 0.0, g.numel(), _dt(g))
        return dx, None, None


def affine(x: Tensor, a: float, c: float) -> Tensor:
    return _AffineFn.apply(x, float(a), float(c))


class _MulFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x = _c(x); y = _c(y)
        out = torch.empty_like(x)
        call("hdmoe_mul", out, x, y, x.numel(), _dt(x))
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = _c(g)
        dx = dy = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(g); call("hdmoe_mul", dx, g, y, g.numel(), _dt(g))
        if ctx.needs_input_grad[1]:
            dy = torch.empty_like(g); call("hdmoe_mul", dy, g, x, g.numel(), _dt(g))
        return dx, dy


def mul(x: Tensor, y: Tensor) -> Tensor:
    return _MulFn.apply(x, y)


class _CastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        x = _c(x)
        ctx.src = x.dtype
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
        call("hdmoe_cast", out, x, x.numel(), dtype_code_cast(x.dtype), dtype_code_cast(dtype))
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        dx = torch.empty(g.shape, dtype=ctx.src, device=g.device)
        call("hdmoe_cast", dx, g, g.numel(), dtype_code_cast(g.dtype), dtype_code_cast(ctx.src))
        return dx, None


def cast(x: Tensor, dtype: torch.dtype) -> Tensor:
    """Element type conversion.  float16 is accepted at the module boundary only (fp16 <-> fp32; the kernels compute in fp32 / bf16)."""
    if x.dtype == dtype:
        return x
    if torch.float16 in (x.dtype, dtype) and torch.bfloat16 in (x.dtype, dtype):
        return _CastFn.apply(_CastFn.apply(x, torch.float32), dtype)
    return _CastFn.apply(x, dtype)


def f32_params(ts):
    """fp16 parameters (a module after `.half()`) as fp32 tensors for the kernels; gradients flow back in fp16."""
    return [cast(t, torch.float32) if torch.is_tensor(t) and t.dtype == torch.float16 else t for t in ts]


class _MPSiluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        out = torch.empty_like(x)
        call("hdmoe_mp_silu_fwd", out, x, x.numel(), _dt(x))
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _c(g)
        dx = torch.empty_like(x)
        call("hdmoe_mp_silu_bwd", dx, g, x, x.numel(), _dt(x))
        return dx


def mp_silu(x: Tensor) -> Tensor:
    return _MPSiluFn.apply(x)


class _SigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a):
        x = _c(x)
        out = torch.empty_like(x)
        call("hdmoe_sigmoid_fwd", out, x, a, x.numel(), _dt(x))
        ctx.save_for_backward(out)
        ctx.a = a
        return out

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _c(g)
        dx = torch.empty_like(y)
        call("hdmoe_sigmoid_bwd", dx, g, y, ctx.a, y.numel(), _dt(y))
        return dx, None


def sigmoid(x: Tensor, a: float = 1.0) -> Tensor:
    """sigmoid(a * x)."""
    return _SigmoidFn.apply(x, float(a))


class _FilmRec:
    """What the consumer of h = film_silu(u, e) needs to run the FiLM backward itself: the saved pre-activation, the embedding, the keep
    bytes of the dropout (None: p == 0) -- attached to h as ``h._film_rec``.  A conv layer that reads h registers in its forward; in its
    backward the bwd7 launch writes du / de in its dgrad epilogue and offers them, and the FiLM node claims them and hands them on without a
    launch.  h must feed that layer alone, as in Unet_block: the FiLM node checks that the gradient it receives is the very tensor the
    conv wrote."""
    __slots__ = ("u", "e", "mask", "p", "taken", "_offer")

    def __init__(self, u, e, mask, p):
        self.u, self.e, self.mask, self.p = u, e, mask, p
        self.taken, self._offer = 0, None

    def register(self) -> None:                              # a conv layer's forward reads h
        self.taken += 1

    def sole_consumer(self, x: Tensor) -> bool:              # may the one registered layer, whose input is x, run the FiLM backward?
        return self.taken == 1 and self.u.shape == x.shape and self.u.dtype == x.dtype

    def clear(self) -> None:    # every backward pass starts clean: one that ended before the FiLM node (autograd.grad(inputs=h)) leaves its offer behind
        self._offer = None

    def offer(self, du: Tensor, de: Tensor) -> None:         # the conv layer's backward launch wrote them
        self._offer = (du, de)

    def claim(self, g: Tensor):
        """The FiLM node's backward, handed ``g``: (du, de) of the consumer's launch -- g is then du -- or None: the node runs its own kernel."""
        offer, self._offer = self._offer, None
        if offer is not None and (g.data_ptr() != offer[0].data_ptr() or g.shape != offer[0].shape):
            raise RuntimeError("film_silu: the output fed a second consumer beside the conv layer that fused its backward (set ops.FILM_DGRAD = False)")
        return offer


FILM_MASK = True                                        # False: the FiLM backward draws the dropout bits again instead of reading saved keep bytes
FILM_DGRAD = True                                       # False: the FiLM backward always runs as its own launch


def _film_record(ctx, out, u, e, mask, p):
    ctx.rec = None
    if u.dtype == torch.bfloat16 and u.ndim == 4 and (p == 0.0 or mask is not None):
        ctx.rec = out._film_rec = _FilmRec(u, e, mask, p)


class _FilmSiluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, e, p, seed):
        ctx.pool_ok = not e.is_leaf
        u = _c(u); e = _f32(e)
        N, C = u.shape[0], u.shape[-1]
        HW = u.numel() // (N * C)
        out = torch.empty_like(u)
        mask = None
        if p > 0.0 and FILM_MASK and u.dtype == torch.bfloat16 and C % 8 == 0:
            # one keep bit per element beside the output: the backward (its own launch, or the consumer's dgrad epilogue) never draws
            mask = torch.empty(u.numel() // 8, dtype=torch.uint8, device=u.device)
            call("hdmoe_film_silu_drop_fwd_mask", out, mask, u, e, N, HW, C, seed, step_counter(u.device), p, _dt(u))
        elif p > 0.0:
            call("hdmoe_film_silu_drop_fwd", out, u, e, N, HW, C, seed, step_counter(u.device), p, _dt(u))
        else:
            call("hdmoe_film_silu_fwd", out, u, e, N, HW, C, _dt(u))
        ctx.save_for_backward(u, e)
        ctx.meta = (p, seed)
        ctx.mask = mask
        _film_record(ctx, out, u, e, mask, p)
        return out

    @staticmethod
    def backward(ctx, g):
        u, e = ctx.saved_tensors
        p, seed = ctx.meta
        rec, mask = getattr(ctx, "rec", None), getattr(ctx, "mask", None)
        done = rec.claim(g) if rec is not None else None
        if done is not None:                                  # the consumer's backward launch already applied this node's backward: g is du
            return g, done[1], None, None
        g = _c(g)
        N, C = u.shape[0], u.shape[-1]
        HW = u.numel() // (N * C)
        du = torch.empty_like(u)
        de = _zeros(e.shape, e.dtype, e.device, ctx.pool_ok)
        if p > 0.0 and mask is not None:
            call("hdmoe_film_silu_mask_bwd", du, de, g, u, e, mask, N, HW, C, p, _dt(u))
        elif p > 0.0:
            call("hdmoe_film_silu_drop_bwd", du, de, g, u, e, N, HW, C, seed, step_counter(u.device), p, _dt(u))
        else:
            call("hdmoe_film_silu_bwd", du, de, g, u, e, N, HW, C, _dt(u))
        return du, de, None, None


class _FilmReq:
    """ops.mp_conv_film's request to the conv (ops._mp_conv(film=...)): the FiLM operands in, ``h`` out when the conv launch took the epilogue."""
    __slots__ = ("emb", "p", "seed", "h")

    def __init__(self, emb, p, seed):
        self.emb, self.p, self.seed, self.h = emb, p, seed, None


CONV_FILM = True                                       # False: always the separate FiLM pass
CONV_FILM_TRAIN = False                                 # True: the fused FiLM epilogue with dropout too


class _FilmDoneFn(torch.autograd.Function):
    """film_silu whose forward was already computed by the producing conv's epilogue (h): only the backward is left."""

    @staticmethod
    def forward(ctx, u, e, p, seed, h):
        ctx.pool_ok = not e.is_leaf
        ctx.save_for_backward(u, e)
        ctx.meta = (p, seed)
        out = h.view_as(h)
        _film_record(ctx, out, u, e, None, p)                 # (the producing launch saved no keep bytes: a record only without dropout)
        return out

    @staticmethod
    def backward(ctx, g):
        return _FilmSiluFn.backward(ctx, g) + (None,)


def mp_conv_film(x: Tensor, weights, gain, emb: Tensor, p: float, training: bool, seg: Optional[Tensor] = None) -> Tensor:
    """film_silu(mp_conv(x, weights, gain), emb, p) -- conv_res1 of Unet_block followed by FiLM, mp_silu and dropout (reference
    model_components.py:240-246).  In the bf16 bank path the second step is an extra output of the conv kernel's epilogue.
    With ops.FILM_DGRAD the result may feed ONE conv layer and nothing else that needs its gradient (see ops.film_silu)."""
    p = float(p) if training else 0.0
    C = int((weights[0] if isinstance(weights, (list, tuple)) else weights).shape[0])
    # Only without dropout (eval / sampling), unless forced (CONV_FILM_TRAIN): drawing the Philox bits in the conv epilogue -- 8 waves per CU,
    # on every unit's critical path -- costs more than the whole separate pass (measured: conv6<2,1> 44 -> 85 us against a 22-us film kernel).
    ok = (CONV_FILM and (p == 0.0 or CONV_FILM_TRAIN) and x.dtype == torch.bfloat16 and x.ndim == 4 and C % 8 == 0 and 256 % (C // 8) == 0
          and _bank.ACTIVE is not None)
    if not ok:
        return film_silu(mp_conv(x, weights, gain, seg=seg, training=training), emb, p, training)
    req = _FilmReq(_f32(emb), p, _next_seed() if p > 0.0 else 0)
    y = _mp_conv(x, weights, gain, seg=seg, training=training, film=req)
    if req.h is not None:
        return _FilmDoneFn.apply(y, req.emb, p, req.seed, req.h)
    return _FilmSiluFn.apply(y, req.emb, p, req.seed)


ONES6 = True                                                # the 33-channel first conv of Unet_expert on conv6 / wgrad6 (csrc/ones6.hip)
BLK6 = True
# Which blocks take the fused launch.  Measured per layer shape (tools/blk6_bench.py, graph replay, N = 512 rows, experts [3,3,5,5],
# dropout 0.2; fused vs conv6 + film_silu + conv6): 32 -> 32 at 32x32 108 vs 117 us, 64 -> 32 140 vs 142, 32 -> 32 at 16x16 33 vs 42; but
# 64 -> 64 at 16x16 76 vs 73, 128 -> 64 98 vs 93, 64 -> 64 at 32x32 306 vs 280: with 64 output channels the unit's phases (conv A, middle op,
# conv B) run one after the other in a single 8-wave workgroup and the halo recompute is not paid back.  "c32": 32-channel blocks only.
# Round 4: on 32 x 32 maps with enough routed rows the whole-image streaming kernel (csrc/conv7.hip) runs the two convs + the FiLM pass in
# 2 x 27 + 19 us against the fused launch's 97-108 us, so "c32" leaves those blocks to it (same box: 14.00 -> 13.72 ms / step).
BLK6_SCOPE = "c32"


def unet_block_fused(h: Tensor, res: Optional[Tensor], w1s, w2s, gain1: float, gain2: float, emb: Tensor, p: float, training: bool,
                     seg: Optional[Tensor], alpha: float, beta: float, res_grad_raw: bool = False) -> Optional[Tensor]:
    """Main branch of Unet_block (reference model_components.py:240-253) for a bank of experts as ONE launch (csrc/blk6.hip):
    alpha * conv_res2(dropout(mp_silu(conv_res1(h) * emb))) + beta * res, the activation tile kept in LDS between the two convs.
    Returns None when the fused kernel does not apply (no ready weight-bank entries, fp32 mode, shapes outside its domain): the caller
    then runs the layers one by one.  The autograd graph is the unfused one (conv -> FiLM -> conv nodes over the tensors the fused
    launch wrote), so the backward is unchanged."""
    w1s, w2s = list(w1s), list(w2s)
    if not (BLK6 and _bank.ACTIVE is not None and _prof_ok() and h.dtype == torch.bfloat16 and h.ndim == 4 and h.is_cuda):
        return None
    if res is not None and (res.dtype != h.dtype or not res.is_contiguous()):
        return None
    ent1 = _bank.ACTIVE.lookup(w1s, h.dtype, float(gain1), 1.0, True)
    ent2 = _bank.ACTIVE.lookup(w2s, h.dtype, float(gain2), float(alpha), True)
    if ent1 is None or ent2 is None or ent1.khs != ent1.kws or ent1.khs != ent2.khs or ent2.khs != ent2.kws:
        return None
    h = _c(h)
    N, H, W, Cin = h.shape
    C = ent1.O
    if ent1.I != Cin or ent2.I != C or ent2.O != C or (seg is None and len(w1s) != 1):
        return None
    if BLK6_SCOPE == "c32" and (C != 32 or (H == 32 and W == 32 and N >= _c7_min_images())):
        return None
    p = float(p) if training else 0.0
    e32 = _f32(emb)
    seed = _next_seed() if p > 0.0 else 0
    y = torch.empty((N, H, W, C), dtype=h.dtype, device=h.device)
    need_bwd = torch.is_grad_enabled() and (h.requires_grad or emb.requires_grad or any(w.requires_grad for w in w1s + w2s))
    # (inference: the pre-activation and the activation are not written at all -- two of the launch's three output streams)
    u = torch.empty_like(y) if need_bwd else None
    hb = torch.empty_like(y) if need_bwd else None
    if _timed("fused", dict(name="blk6_kernel (fwd)", dtype="bfloat16", seg=seg, N=N, HW=H * W, O=C, I=Cin + C, taps=[k * k for k in ent1.khs], mult=1.0),
              "hdmoe_unet_block_fwd", h, ent1.wf, ent2.wf, u, hb, y, res, e32, seed, step_counter(h.device), p, float(alpha), float(beta), seg,
              len(w1s), ent1.wstride, ent2.wstride, N, H, W, Cin, C, ent1.khs, _dt(h)) != 0:
        if p > 0.0:
            _seed_state["ctr"] -= 1                            # nothing was launched: the unfused path draws this salt itself
        return None
    STATS["blk"] += 1
    if not need_bwd:
        return y
    ws1 = w1s if seg is not None else w1s[0]
    ws2 = w2s if seg is not None else w2s[0]
    uu = _mp_conv(h, ws1, gain1, seg=seg, training=training, out=u)
    hh = _FilmDoneFn.apply(uu, e32, p, seed, hb)
    return _mp_conv(hh, ws2, gain2, seg=seg, res=res, alpha=alpha, beta=beta, training=training, res_grad_raw=res_grad_raw, out=y)


def film_silu(u: Tensor, e: Tensor, p: float = 0.0, training: bool = False) -> Tensor:
    """dropout_p(mp_silu(u * e[n, c])) with e a float32 (N, C) embedding (model_components.py:242-246); the dropout is fused
    into the same pass when the layout is 16-byte vectorisable, otherwise it runs as a separate kernel.
    With ops.FILM_DGRAD (default) a bf16 result that feeds a k x k bank conv layer has its backward run in that layer's backward launch
    (ops._FilmRec): the result must then feed that layer alone -- a second consumer that is a conv layer falls back to this node's own
    kernel, any other second consumer raises in the backward.  Set ops.FILM_DGRAD = False for such a graph."""
    p = float(p) if training else 0.0
    C = u.shape[-1]
    vw = 16 // u.element_size()
    if p > 0.0 and not (C % vw == 0 and 256 % (C // vw) == 0):
        return dropout(_FilmSiluFn.apply(u, e, 0.0, 0), p, True)
    return _FilmSiluFn.apply(u, e, p, _next_seed() if p > 0.0 else 0)


class _ScaleRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.pool_ok = not s.is_leaf
        x = _c(x); s = _f32(s).reshape(-1)
        rows = x.shape[0]
        L = x.numel() // rows
        out = torch.empty_like(x)
        call("hdmoe_scale_rows_fwd", out, x, s, rows, L, _dt(x))
        ctx.save_for_backward(x, s)
        return out

    @staticmethod
    def backward(ctx, g):
        x, s = ctx.saved_tensors
        g = _c(g)
        rows = x.shape[0]
        L = x.numel() // rows
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ds = _zeros(s.shape, s.dtype, s.device, ctx.pool_ok) if ctx.needs_input_grad[1] else None
        call("hdmoe_scale_rows_bwd", dx, ds, g, x, s, rows, L, _dt(x))
        return dx, ds


def scale_rows(x: Tensor, s: Tensor) -> Tensor:
    """out[n] = s[n] * x[n] with s a float32 (N,) vector."""
    return _ScaleRowsFn.apply(x, s)


class _Cat2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, wa, wb):
        a = _c(a); b = _c(b)
        Ca, Cb = a.shape[-1], b.shape[-1]
        rows = a.numel() // Ca
        out = torch.empty((*a.shape[:-1], Ca + Cb), dtype=a.dtype, device=a.device)
        call("hdmoe_cat2_fwd", out, a, b, wa, wb, Ca, Cb, rows, _dt(a))
        ctx.meta = (wa, wb, a.shape, b.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        wa, wb, sa, sb = ctx.meta
        g = _c(g)
        da = torch.empty(sa, dtype=g.dtype, device=g.device)
        db = torch.empty(sb, dtype=g.dtype, device=g.device)
        call("hdmoe_cat2_bwd", da, db, g, wa, wb, sa[-1], sb[-1], da.numel() // sa[-1], _dt(g))
        return da, db, None, None


def mp_cat(a: Tensor, b: Tensor, t: float = 0.5) -> Tensor:
    """Channel-last mp_cat (model_internals.py:69-92)."""
    na, nb = a.shape[-1], b.shape[-1]
    c = math.sqrt((na + nb) / ((1.0 - t) ** 2 + t ** 2))
    return _Cat2Fn.apply(a, b, c * (1.0 - t) / math.sqrt(na), c * t / math.sqrt(nb))


class _SiluBranchFn(torch.autograd.Function):
    """x -> (x, mp_silu(x)) for a tensor that feeds mp_silu and a second consumer (decoder-block input: skip / residual path).
    Backward: ONE pass, dx = gx + gh * mp_silu'(x) (instead of mp_silu_bwd + a gradient-sum launch)."""

    @staticmethod
    def forward(ctx, x, gx_scale):
        ctx.set_materialize_grads(False)
        x = _c(x)
        h = torch.empty_like(x)
        call("hdmoe_mp_silu_fwd", h, x, x.numel(), _dt(x))
        ctx.save_for_backward(x)
        ctx.sx = float(gx_scale)
        return x.view(x.shape), h

    @staticmethod
    def backward(ctx, gx, gh):
        (x,) = ctx.saved_tensors
        if gh is None:
            if gx is None or ctx.sx == 1.0:
                return gx, None
            dx = torch.empty_like(x)
            call("hdmoe_axpby", dx, _c(gx), None, ctx.sx, 0.0, dx.numel(), _dt(dx))
            return dx, None
        gh = _c(gh)
        dx = torch.empty_like(x)
        if gx is None:
            call("hdmoe_mp_silu_bwd", dx, gh, x, x.numel(), _dt(x))
        else:
            call("hdmoe_mp_silu_bwd_add", dx, gh, x, _c(gx), ctx.sx, x.numel(), _dt(x))
        return dx, None


class _CatSiluFn(torch.autograd.Function):
    """(mp_cat(a, b), mp_silu(mp_cat(a, b))) in one pass; backward in one pass as well."""

    @staticmethod
    def forward(ctx, a, b, wa, wb):
        ctx.set_materialize_grads(False)
        a = _c(a); b = _c(b)
        Ca, Cb = a.shape[-1], b.shape[-1]
        out = torch.empty((*a.shape[:-1], Ca + Cb), dtype=a.dtype, device=a.device)
        h = torch.empty_like(out)
        call("hdmoe_cat2_silu_fwd", out, h, a, b, wa, wb, Ca, Cb, a.numel() // Ca, _dt(a))
        ctx.save_for_backward(out)
        ctx.meta = (wa, wb, a.shape, b.shape)
        return out, h

    @staticmethod
    def backward(ctx, gcat, gh):
        (out,) = ctx.saved_tensors
        wa, wb, sa, sb = ctx.meta
        da = torch.empty(sa, dtype=out.dtype, device=out.device)
        db = torch.empty(sb, dtype=out.dtype, device=out.device)
        if gh is None:
            if gcat is None:
                return None, None, None, None
            call("hdmoe_cat2_bwd", da, db, _c(gcat), wa, wb, sa[-1], sb[-1], da.numel() // sa[-1], _dt(out))
        else:
            call("hdmoe_cat2_silu_bwd", da, db, None if gcat is None else _c(gcat), _c(gh), out, wa, wb, sa[-1], sb[-1], da.numel() // sa[-1], _dt(out))
        return da, db, None, None


def _vec_ok(*ts) -> bool:
    return all(t.shape[-1] % (8 if t.dtype == torch.bfloat16 else 4) == 0 and t.dtype in (torch.bfloat16, torch.float32) for t in ts)


def silu_branch(x: Tensor, gx_scale: float = 1.0):
    """(x, mp_silu(x)): the pair a decoder block needs (x continues on the skip / residual path).  ``gx_scale``: factor applied to
    the gradient arriving for the returned x (see mp_conv(res_grad_raw=True))."""
    if _vec_ok(x) and x.numel() % 8 == 0:
        return _SiluBranchFn.apply(x, float(gx_scale))
    x, xh = fanout(x, 2)
    if gx_scale != 1.0:
        x = affine_grad(x, gx_scale)
    return x, mp_silu(xh)


class _GradScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        dx = torch.empty_like(g)
        call("hdmoe_axpby", dx, g, None, ctx.s, 0.0, g.numel(), _dt(g))
        return dx, None


def affine_grad(x: Tensor, s: float) -> Tensor:
    """Identity in the forward, gradient times ``s`` in the backward (the unfused form of a deferred residual-gradient scale)."""
    return _GradScaleFn.apply(x, float(s))


def mp_cat_silu(a: Tensor, b: Tensor, t: float = 0.5):
    """(mp_cat(a, b, t), mp_silu of it) in one pass (model_internals.py:69-92 followed by :33-36)."""
    if not (_vec_ok(a, b) and a.dtype == b.dtype):
        return silu_branch(mp_cat(a, b, t))
    na, nb = a.shape[-1], b.shape[-1]
    c = math.sqrt((na + nb) / ((1.0 - t) ** 2 + t ** 2))
    return _CatSiluFn.apply(a, b, c * (1.0 - t) / math.sqrt(na), c * t / math.sqrt(nb))


class _ResampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        x = _c(x)
        N, H, W, C = x.shape
        ctx.mode = mode
        if mode == "down":
            out = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
            call("hdmoe_pool2", out, x, N, H // 2, W // 2, C, 0.25, _dt(x))
        else:
            out = torch.empty((N, H * 2, W * 2, C), dtype=x.dtype, device=x.device)
            call("hdmoe_upsample2", out, x, N, H * 2, W * 2, C, 1.0, _dt(x))
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        N, H, W, C = g.shape
        if ctx.mode == "down":
            dx = torch.empty((N, H * 2, W * 2, C), dtype=g.dtype, device=g.device)
            call("hdmoe_upsample2", dx, g, N, H * 2, W * 2, C, 0.25, _dt(g))
        else:
            dx = torch.empty((N, H // 2, W // 2, C), dtype=g.dtype, device=g.device)
            call("hdmoe_pool2", dx, g, N, H // 2, W // 2, C, 1.0, _dt(g))
        return dx, None


class _FirResampleFn(torch.autograd.Function):
    """resample(x, f, mode) for an even-length filter other than [1, 1] (model_internals.py:95-127): depthwise stride-2 correlation
    with outer(f, f) / f.sum()^2 ('down') or its transpose with 4x the taps ('up'); each is the other's backward."""

    @staticmethod
    def forward(ctx, x, taps, mode):
        x = _c(x)
        N, H, W, C = x.shape
        L = len(taps)
        pad = (L - 1) // 2
        if mode == "down":
            Ho, Wo = (H + 2 * pad - L) // 2 + 1, (W + 2 * pad - L) // 2 + 1
            out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
            call("hdmoe_fir_resample", out, x, taps, L, pad, 1.0, 0, N, H, W, Ho, Wo, C, _dt(x))
        else:
            Ho, Wo = (H - 1) * 2 - 2 * pad + L, (W - 1) * 2 - 2 * pad + L
            out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
            call("hdmoe_fir_resample", out, x, taps, L, pad, 4.0, 1, N, H, W, Ho, Wo, C, _dt(x))
        ctx.meta = (taps, mode, L, pad, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        taps, mode, L, pad, H, W = ctx.meta
        g = _c(g)
        N, Hg, Wg, C = g.shape
        dx = torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
        if mode == "down":                                     # transpose of the strided correlation (no 4x)
            call("hdmoe_fir_resample", dx, g, taps, L, pad, 1.0, 1, N, Hg, Wg, H, W, C, _dt(g))
        else:
            call("hdmoe_fir_resample", dx, g, taps, L, pad, 4.0, 0, N, Hg, Wg, H, W, C, _dt(g))
        return dx, None, None


def resample(x: Tensor, mode: str = "keep", f=(1, 1)) -> Tensor:
    """resample (model_internals.py:95-127), channel-last.  f = [1, 1]: 'down' = 2x2 mean, 'up' = nearest x2 (vector kernels);
    any other even-length filter with up to 8 taps: the generic separable FIR kernels."""
    if mode == "keep":
        return x
    if mode not in ("down", "up"):
        raise ValueError(f"Invalid mode: {mode}")
    f = [float(v) for v in f]
    if len(f) % 2 or not f:
        raise AssertionError("resample: the filter must be 1-D with an even number of taps")
    if f == [1.0, 1.0] and not (mode == "down" and (x.shape[1] % 2 or x.shape[2] % 2)):
        return _ResampleFn.apply(x, mode)
    if len(f) > 8:
        raise NotImplementedError("resample: filters with more than 8 taps are not implemented")
    tot = sum(f)
    return _FirResampleFn.apply(x, tuple(v / tot for v in f), mode)


class _SeqReduceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = _c(x)
        N, C = x.shape[0], x.shape[-1]
        S = x.numel() // (N * C)
        out = torch.zeros((N, C), dtype=torch.float32, device=x.device)
        call("hdmoe_seq_reduce", out, x, N, S, C, scale, _dt(x))
        ctx.meta = (x.shape, x.dtype, scale, S)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, dt, scale, S = ctx.meta
        g = _f32(g)
        dx = torch.empty(shape, dtype=dt, device=g.device)
        call("hdmoe_seq_bcast_add", dx, None, g, shape[0], S, shape[-1], scale, dtype_code(dt))
        return dx, None


def seq_mean(x: Tensor) -> Tensor:
    """Mean over all middle dims: (N, ..., C) -> float32 (N, C)  (AdaptiveAvgPool2d(1) / text.mean(1))."""
    N, C = x.shape[0], x.shape[-1]
    return _SeqReduceFn.apply(x, 1.0 / (x.numel() // (N * C)))


class _SeqBcastAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        ctx.pool_ok = not t.is_leaf
        x = _c(x); t = _f32(t)
        N, C = x.shape[0], x.shape[-1]
        S = x.numel() // (N * C)
        out = torch.empty_like(x)
        call("hdmoe_seq_bcast_add", out, x, t, N, S, C, 1.0, _dt(x))
        ctx.meta = (N, S, C)
        return out

    @staticmethod
    def backward(ctx, g):
        N, S, C = ctx.meta
        g = _c(g)
        dt_ = None
        if ctx.needs_input_grad[1]:
            dt_ = _zeros((N, C), torch.float32, g.device, ctx.pool_ok)
            call("hdmoe_seq_reduce", dt_, g, N, S, C, 1.0, _dt(g))
        return g, dt_


def seq_bcast_add(x: Tensor, t: Tensor) -> Tensor:
    """x[n, s, :] + t[n, :] (the q/k/v time biases of MP_Attention, model_internals.py:368-372)."""
    return _SeqBcastAddFn.apply(x, t)


class _BiasAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        x = _c(x); bias = _f32(bias)
        L = bias.numel()
        out = torch.empty_like(x)
        call("hdmoe_bias_add", out, x, bias, x.numel() // L, L, _dt(x))
        ctx.bshape = bias.shape
        ctx.bias_param = bias if (bias.is_leaf and bias.requires_grad) else None
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        db = None
        if ctx.needs_input_grad[1]:
            L = 1
            for d in ctx.bshape:
                L *= d
            bp = ctx.bias_param
            if _direct(bp):
                call("hdmoe_colsum", bp.grad, g, g.numel() // L, L, _dt(g))
            else:
                db = torch.zeros(ctx.bshape, dtype=torch.float32, device=g.device)
                call("hdmoe_colsum", db, g, g.numel() // L, L, _dt(g))
        return g, db


def bias_add(x: Tensor, bias: Tensor) -> Tensor:
    """x viewed as (rows, bias.numel()) + bias (pos_emb add, model_components.py:680)."""
    return _BiasAddFn.apply(x, bias)


class _LerpParamFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha):
        a = _c(a); b = _c(b)
        out = torch.empty_like(a)
        call("hdmoe_lerp_param_fwd", out, a, b, alpha, a.numel(), _dt(a))
        ctx.save_for_backward(a, b, alpha)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, alpha = ctx.saved_tensors
        g = _c(g)
        da, db = torch.empty_like(a), torch.empty_like(b)
        direct = _direct(alpha)
        dal = alpha.grad if direct else torch.zeros_like(alpha)
        call("hdmoe_lerp_param_bwd", da, db, dal, g, a, b, alpha, a.numel(), _dt(a))
        return da, db, (None if direct else dal)


def lerp_param(a: Tensor, b: Tensor, alpha: Tensor) -> Tensor:
    """a + alpha*(b - a) with a learnable float32 scalar (model_config2.py:291)."""
    return _LerpParamFn.apply(a, b, alpha)


class _GateMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, U, A):
        logits = _c(logits); U = _c(U); A = _c(A)
        C = U.shape[-1]
        rows = U.numel() // C
        out = torch.empty_like(U)
        gate = torch.empty((*U.shape[:-1], 2), dtype=torch.float32, device=U.device)
        call("hdmoe_gate_mix_fwd", out, gate, logits, U, A, rows, C, _dt(U))
        ctx.save_for_backward(gate, U, A)
        return out, gate

    @staticmethod
    def backward(ctx, g, dgate):
        gate, U, A = ctx.saved_tensors
        g = _c(g)
        dgate = None if dgate is None else _f32(dgate)
        C = U.shape[-1]
        rows = U.numel() // C
        dU, dA = torch.empty_like(U), torch.empty_like(A)
        dl = torch.empty((*U.shape[:-1], 2), dtype=U.dtype, device=U.device)
        call("hdmoe_gate_mix_bwd", dU, dA, dl, g, dgate, gate, U, A, rows, C, _dt(U))
        return dl, dU, dA


def gate_mix(logits: Tensor, U: Tensor, A: Tensor):
    """softmax gate over 2 channels + mix + mp_sum (model_config2.py:297-301).  Returns (out, gate fp32)."""
    return _GateMixFn.apply(logits, U, A)


# ---- fusion stage: the token-local chain in front of the first attention call, one launch per direction (csrc/fusion.hip)
FUSION_FUSED = True                                     # False: always the unfused chain (axpby, scale_rows, three mp_conv)


class _FusionInFn(torch.autograd.Function):
    """(query, ctx, q, k, v) = hdmoe_fusion_in_fwd(fu, fv, sw) with the prepared images of the weight-bank entries ``ents`` (q, k, v
    projection); without ``sw`` query and ctx are fu and fv themselves.  The backward is ONE launch: hdmoe_fusion_in_bwd_wg for dfu, dfv
    and dsw -- the gradient fan-in of query and ctx included -- and the three projections' weight gradients, contracted from the rows the
    kernel holds (query and ctx recomputed from fu, fv, sw) straight into the bank's slabs; hdmoe_fusion_in_bwd when no weight wants one."""

    @staticmethod
    def forward(ctx, fu, fv, sw, ents, S, *weights):
        ctx.set_materialize_grads(False)
        rows = fu.numel() // 32
        query, cx = (torch.empty_like(fu), torch.empty_like(fu)) if sw is not None else (None, None)
        q, k, v = torch.empty_like(fu), torch.empty_like(fu), torch.empty_like(fu)
        if call("hdmoe_fusion_in_fwd", fu, fv, sw, ents[0].wf, ents[1].wf, ents[2].wf, query, cx, q, k, v, rows, S, 32,
                ents[0].alpha, ents[1].alpha, ents[2].alpha, BF16) != 0:
            raise RuntimeError("hdmoe_fusion_in_fwd declined a call that ops.fusion_in admitted")
        ctx.ents, ctx.bank, ctx.S, ctx.pool_ok = ents, _bank.ACTIVE, S, sw is not None and not sw.is_leaf
        ctx.save_for_backward(fu, fv, *(() if sw is None else (sw,)))     # (the backward recomputes query and ctx from these)
        STATS["fusion_in"] += 1
        return (fu, fv, q, k, v) if sw is None else (query, cx, q, k, v)

    @staticmethod
    def backward(ctx, gquery, gctx, gq, gk, gv):
        fu, fv, *rest = ctx.saved_tensors
        sw = rest[0] if rest else None
        ents, rows = ctx.ents, fu.numel() // 32
        gq, gk, gv = (torch.zeros_like(fu) if g is None else _c(g) for g in (gq, gk, gv))
        dfu, dfv = torch.empty_like(fu), torch.empty_like(fv)
        dsw = None if sw is None else _zeros(sw.shape, torch.float32, sw.device, ctx.pool_ok)
        head = (gq, gk, gv, _c(gquery), _c(gctx), fu, fv, sw, ents[0].wd, ents[1].wd, ents[2].wd, dfu, dfv, dsw)
        tail = (rows, ctx.S, 32, ents[0].alpha, ents[1].alpha, ents[2].alpha, BF16)
        if any(ctx.needs_input_grad[5:]):
            # with the weight gradients, straight into the bank's slabs (finished with every other layer's)
            if call("hdmoe_fusion_in_bwd_wg", *head, ents[0].G[0], ents[1].G[0], ents[2].G[0], 0, *tail) != 0:
                raise RuntimeError("hdmoe_fusion_in_bwd_wg declined a call whose forward ran fused")
            for ent in ents:
                ctx.bank.note_backward(ent)
        elif call("hdmoe_fusion_in_bwd", *head, *tail) != 0:
            raise RuntimeError("hdmoe_fusion_in_bwd declined a call whose forward ran fused")
        return (dfu, dfv, dsw, None, None) + (None,) * len(ents)


def fusion_in(fu: Tensor, fv: Tensor, sw: Optional[Tensor], projs, gain: float = 1.0):
    """The head of the fusion stage in one launch: query = fu + sw (fv - fu), ctx = fv - sw (fv - fu) (``sw``: (B,) float32, or None --
    then query, ctx = fu, fv) and q, k, v = the three pointwise projections ``projs`` (weight tensors, plain ``gain``) of query, ctx,
    ctx.  fu, fv: (B, S, 32).  Returns (query, ctx, q, k, v), or None outside the fused kernel's domain (bf16 rows of 32 channels,
    16-byte aligned, every projection a ready weight-bank entry): the caller then runs the unfused ops."""
    bank = _bank.ACTIVE
    if not (FUSION_FUSED and _prof_ok() and bank is not None and fu.is_cuda and fu.ndim == 3 and fu.shape == fv.shape and fu.shape[-1] == 32
            and fu.dtype == fv.dtype == torch.bfloat16 and fu.is_contiguous() and fv.is_contiguous()
            and fu.data_ptr() % 16 == 0 and fv.data_ptr() % 16 == 0 and fu.numel() > 0):
        return None
    if sw is not None and not (sw.dtype == torch.float32 and sw.numel() == fu.shape[0] and sw.is_contiguous()):
        return None
    ws = f32_params(list(projs))
    if not all(w.shape[0] == 32 and w.shape[1] == 32 and _kernel_hw(w) == (1, 1) for w in ws):
        return None
    ents = [bank.lookup([w], torch.bfloat16, float(gain), 1.0, True) for w in ws]      # (the key ops.mp_conv registers the layer under)
    if any(e is None for e in ents):
        return None
    return _FusionInFn.apply(fu, fv, sw, ents, int(fu.shape[1]), *ws)


class _FusionOutFn(torch.autograd.Function):
    """(mixed, gate) = hdmoe_fusion_out_fwd(o2, a, U): out_proj of the text cross-attention with its residual, lerp_param, mp_cat, gate1,
    mp_silu, gate2 and gate_mix.  ``ents``: the bank entries of out_proj, gate1, gate2; ``k`` = (alpha_o, beta_o, wa, wb).  The backward
    is ONE launch: hdmoe_fusion_out_bwd_wg (do2, da, dU, dalpha and the three layers' weight gradients into the bank's slabs; their dy
    never leave the kernel and their x, cat and s, are recomputed from U, a2, g1 -- so the forward saves a2 and g1 alone);
    hdmoe_fusion_out_bwd when no weight wants a gradient."""

    @staticmethod
    def forward(ctx, o2, a, U, alpha_txt, ents, k, *weights):
        ctx.set_materialize_grads(False)
        rows = o2.numel() // 32
        mixed = torch.empty_like(U)
        a2 = g1 = None
        if any(ctx.needs_input_grad):                          # (else: inference, nothing is saved)
            a2, g1 = torch.empty_like(U), torch.empty_like(U)
        gate = torch.empty((*U.shape[:-1], 2), dtype=torch.float32, device=U.device)
        consts = (*k, ents[1].alpha, ents[2].alpha)
        if call("hdmoe_fusion_out_fwd", o2, a, U, alpha_txt, ents[0].wf, ents[1].wf, ents[2].wf, mixed, gate, a2, g1, None, None, rows, 32,
                *consts, BF16) != 0:
            raise RuntimeError("hdmoe_fusion_out_fwd declined a call that ops.fusion_out admitted")
        ctx.ents, ctx.bank, ctx.consts = ents, _bank.ACTIVE, consts
        if a2 is not None:
            ctx.save_for_backward(o2, a, U, alpha_txt, a2, g1, gate)
        STATS["fusion_out"] += 1
        return mixed, gate

    @staticmethod
    def backward(ctx, dmixed, dgate):
        o2, a, U, alpha_txt, a2, g1, gate = ctx.saved_tensors
        ents, rows = ctx.ents, o2.numel() // 32
        dmixed = torch.zeros_like(U) if dmixed is None else _c(dmixed)
        dgate = None if dgate is None else _f32(dgate)
        do2, da, dU = torch.empty_like(o2), torch.empty_like(a), torch.empty_like(U)
        direct = _direct(alpha_txt)
        dal = alpha_txt.grad if direct else torch.zeros_like(alpha_txt)
        head = (dmixed, dgate, gate, U, a2, g1, o2, a, alpha_txt, ents[0].wf, ents[0].wd, ents[1].wd, ents[2].wd, do2, da, dU)
        if any(ctx.needs_input_grad[6:]):
            if call("hdmoe_fusion_out_bwd_wg", *head, dal, ents[0].G[0], ents[1].G[0], ents[2].G[0], 0, rows, 32, *ctx.consts, BF16) != 0:
                raise RuntimeError("hdmoe_fusion_out_bwd_wg declined a call whose forward ran fused")
            for ent in ents:
                ctx.bank.note_backward(ent)
        else:
            dat, dg1 = torch.empty_like(o2), torch.empty_like(o2)       # (the dy of weight gradients nobody asked for)
            dl = torch.empty((rows, 2), dtype=U.dtype, device=U.device)
            if call("hdmoe_fusion_out_bwd", *head, dat, dg1, dl, dal, rows, 32, *ctx.consts, BF16) != 0:
                raise RuntimeError("hdmoe_fusion_out_bwd declined a call whose forward ran fused")
        return (do2, da, dU, None if direct else dal, None, None) + (None,) * len(ents)


def fusion_out(o2: Tensor, a: Tensor, U: Tensor, alpha_txt: Tensor, w_out: Tensor, alpha: float, beta: float, w_gate1: Tensor, w_gate2: Tensor,
               gain: float = 1.0):
    """The tail of the fusion stage in one launch: at = out_proj(o2) mixed with the residual ``a`` (alpha, beta as MP_Attention passes them to
    mp_conv), a2 = lerp_param(a, at, alpha_txt), g = gate2(mp_silu(gate1(mp_cat(U, a2, 0.5)))), gate_mix(g, U, a2).  o2, a: (B, S, 32);
    U: (B, H, W, 32).  Returns (mixed, gate) shaped like U, or None outside the fused kernel's domain: the caller then runs the ops."""
    bank = _bank.ACTIVE
    ts = (o2, a, U)
    if not (FUSION_FUSED and _prof_ok() and bank is not None and U.is_cuda and U.shape[-1] == 32 and U.numel() > 0
            and all(t.dtype == torch.bfloat16 and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.numel() == U.numel() for t in ts)
            and alpha_txt.dtype == torch.float32 and alpha_txt.numel() == 1):
        return None
    ws = f32_params([w_out, w_gate1, w_gate2])
    if [tuple(w.shape[:2]) for w in ws] != [(32, 32), (32, 64), (2, 32)] or any(_kernel_hw(w) != (1, 1) for w in ws):
        return None
    ents = [bank.lookup([ws[0]], torch.bfloat16, float(gain), float(alpha), True), bank.lookup([ws[1]], torch.bfloat16, 1.0, 1.0, True),
            bank.lookup([ws[2]], torch.bfloat16, 1.0, 1.0, True)]
    if any(e is None for e in ents):
        return None
    c = math.sqrt(64 / 0.5)                                  # mp_cat(U, a2, 0.5) of two 32-channel tensors
    k = (float(alpha), float(beta), c * 0.5 / math.sqrt(32), c * 0.5 / math.sqrt(32))
    return _FusionOutFn.apply(o2, a, U, alpha_txt, ents, k, *ws)


class _FusionMidFn(torch.autograd.Function):
    """(a, q2) = hdmoe_fusion_mid_fwd(o1, query): out_proj of the first cross-attention with its residual, then q_proj of the text
    attention.  ``ents``: their bank entries; ``k`` = (alpha_o, beta_o).  The backward is one hdmoe_fusion_mid_bwd launch: the gradient
    fan-in of a (no ATen add), do1, the residual's share of query's gradient and both weight gradients into the bank's slabs."""

    @staticmethod
    def forward(ctx, o1, query, ents, k, *weights):
        ctx.set_materialize_grads(False)
        rows = o1.numel() // 32
        a, q2 = torch.empty_like(query), torch.empty_like(query)
        if call("hdmoe_fusion_mid_fwd", o1, query, ents[0].wf, ents[1].wf, a, q2, rows, 32, *k, ents[1].alpha, BF16) != 0:
            raise RuntimeError("hdmoe_fusion_mid_fwd declined a call that ops.fusion_mid admitted")
        ctx.ents, ctx.bank, ctx.k = ents, _bank.ACTIVE, k
        ctx.save_for_backward(o1, a)
        STATS["fusion_mid"] += 1
        return a, q2

    @staticmethod
    def backward(ctx, da, dq2):
        o1, a = ctx.saved_tensors
        ents, rows = ctx.ents, o1.numel() // 32
        da, dq2 = (torch.zeros_like(a) if g is None else _c(g) for g in (da, dq2))
        do1, dres = torch.empty_like(o1), torch.empty_like(a)
        wg = any(ctx.needs_input_grad[4:])
        if call("hdmoe_fusion_mid_bwd", da, dq2, a, o1, ents[0].wd, ents[1].wd, do1, dres, ents[0].G[0] if wg else None,
                ents[1].G[0] if wg else None, 0, rows, 32, *ctx.k, ents[1].alpha, BF16) != 0:
            raise RuntimeError("hdmoe_fusion_mid_bwd declined a call whose forward ran fused")
        if wg:
            for ent in ents:
                ctx.bank.note_backward(ent)
        return (do1, dres, None, None) + (None,) * len(ents)


def fusion_mid(o1: Tensor, query: Tensor, w_out: Tensor, alpha: float, beta: float, w_q: Tensor, gain: float = 1.0):
    """Between the fusion stage's two attention cores in one launch: a = out_proj(o1) mixed with the residual ``query`` (alpha, beta as
    MP_Attention passes them to mp_conv), q2 = q_proj(a) of the text attention.  o1, query: (B, S, 32).  Returns (a, q2), or None outside
    the fused kernel's domain (as ops.fusion_in): the caller then runs the two layers."""
    bank = _bank.ACTIVE
    if not (FUSION_FUSED and _prof_ok() and bank is not None and o1.is_cuda and o1.ndim == 3 and o1.shape == query.shape and o1.shape[-1] == 32
            and o1.dtype == query.dtype == torch.bfloat16 and o1.is_contiguous() and query.is_contiguous()
            and o1.data_ptr() % 16 == 0 and query.data_ptr() % 16 == 0 and o1.numel() > 0):
        return None
    ws = f32_params([w_out, w_q])
    if not all(w.shape[0] == 32 and w.shape[1] == 32 and _kernel_hw(w) == (1, 1) for w in ws) or ws[0].requires_grad != ws[1].requires_grad:
        return None
    ents = [bank.lookup([ws[0]], torch.bfloat16, float(gain), float(alpha), True), bank.lookup([ws[1]], torch.bfloat16, float(gain), 1.0, True)]
    if any(e is None for e in ents):
        return None
    return _FusionMidFn.apply(o1, query, ents, (float(alpha), float(beta)), *ws)


class _KVProjFn(torch.autograd.Function):
    """(k, v) = hdmoe_kgemm2_fwd(x): two 32-output pointwise layers (bank entries ``ents``) over the same wide input, x read once; the
    backward is one hdmoe_lwgrad2 launch into both slabs.  x gets no gradient (ops.kv_proj admits only inputs that want none)."""

    @staticmethod
    def forward(ctx, x, ents, *weights):
        ctx.set_materialize_grads(False)
        rows, K = x.numel() // x.shape[-1], int(x.shape[-1])
        k, v = (torch.empty((*x.shape[:-1], 32), dtype=x.dtype, device=x.device) for _ in range(2))
        if call("hdmoe_kgemm2_fwd", x, ents[0].wf, ents[1].wf, k, v, rows, K, ents[0].alpha, ents[1].alpha, BF16) != 0:
            raise RuntimeError("hdmoe_kgemm2_fwd declined a call that ops.kv_proj admitted")
        ctx.ents, ctx.bank = ents, _bank.ACTIVE
        ctx.save_for_backward(x)
        return k, v

    @staticmethod
    def backward(ctx, gk, gv):
        (x,) = ctx.saved_tensors
        ents, rows, K = ctx.ents, x.numel() // x.shape[-1], int(x.shape[-1])
        if any(ctx.needs_input_grad[2:]):
            gk, gv = (torch.zeros((rows, 32), dtype=x.dtype, device=x.device) if g is None else _c(g) for g in (gk, gv))
            if call("hdmoe_lwgrad2", x, gk, gv, ents[0].G[0], ents[1].G[0], rows, K, BF16) != 0:
                raise RuntimeError("hdmoe_lwgrad2 declined a call whose forward ran fused")
            for ent in ents:
                ctx.bank.note_backward(ent)
        return (None, None) + (None,) * len(ents)


def kv_proj(x: Tensor, w_k: Tensor, w_v: Tensor, gain: float = 1.0):
    """k, v = two pointwise projections (weight tensors, plain ``gain``) of the same x (..., C) in one launch per direction.  Returns (k, v),
    or None outside the domain -- bf16 x that wants no gradient, C % 64 == 0 and >= 512 (the long-contraction kernel's), 32 outputs each,
    both projections ready weight-bank entries: the caller then runs the two layers on their own."""
    bank = _bank.ACTIVE
    if not (FUSION_FUSED and _prof_ok() and bank is not None and x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous()
            and not x.requires_grad and x.numel() > 0 and x.shape[-1] % 64 == 0 and x.shape[-1] >= 512 and x.data_ptr() % 16 == 0):
        return None
    ws = f32_params([w_k, w_v])
    if not all(w.shape[0] == 32 and w.shape[1] == x.shape[-1] and _kernel_hw(w) == (1, 1) for w in ws) or ws[0].requires_grad != ws[1].requires_grad:
        return None
    ents = [bank.lookup([w], torch.bfloat16, float(gain), 1.0, True) for w in ws]      # (the key ops.mp_conv registers the layer under)
    if any(e is None for e in ents):
        return None
    return _KVProjFn.apply(x, ents, *ws)


class _SoftmaxRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = _f32(x)
        out = torch.empty_like(x)
        call("hdmoe_softmax_rows_fwd", out, x, x.numel() // x.shape[-1], x.shape[-1], scale)
        ctx.save_for_backward(out)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(y)
        call("hdmoe_softmax_rows_bwd", dx, g, y, y.numel() // y.shape[-1], y.shape[-1], ctx.scale)
        return dx, None


def softmax_rows(x: Tensor, scale: float = 1.0) -> Tensor:
    return _SoftmaxRowsFn.apply(x, float(scale))


class _AdaLNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cond):
        x = _f32(x); cond = _f32(cond)
        B, F = x.shape
        out = torch.empty_like(x)
        call("hdmoe_adaln_fwd", out, x, cond, B, F)
        ctx.save_for_backward(x, cond)
        return out

    @staticmethod
    def backward(ctx, g):
        x, cond = ctx.saved_tensors
        g = _f32(g)
        B, F = x.shape
        dx, dcond = torch.empty_like(x), torch.empty_like(cond)
        call("hdmoe_adaln_bwd", dx, dcond, g, x, cond, B, F)
        return dx, dcond


def adaln(x: Tensor, cond: Tensor) -> Tensor:
    """x*(1+gamma)+beta with cond = [gamma | beta] (B, 2F) (model_components.py:148-151)."""
    return _AdaLNFn.apply(x, cond)


class _TakeColPosFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, e):
        w = _f32(w)
        B, E = w.shape
        out = torch.empty(B, dtype=torch.float32, device=w.device)
        call("hdmoe_take_col_pos_fwd", out, w, B, E, e)
        ctx.save_for_backward(w)
        ctx.e = e
        return out

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        B, E = w.shape
        dw = torch.zeros_like(w)
        call("hdmoe_take_col_pos_bwd", dw, _f32(g), w, B, E, ctx.e)
        return dw, None


def take_col_pos(w: Tensor, e: int) -> Tensor:
    """(B,) float32: w[:, e] where positive, else 0 (the `out_router[:, i] > 0` mask, model_config1.py:26,35)."""
    return _TakeColPosFn.apply(w, int(e))


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x = _c(x)
        out = torch.empty_like(x)
        call("hdmoe_dropout", out, x, seed, step_counter(x.device), p, x.numel(), _dt(x))
        ctx.meta = (p, seed)
        return out

    @staticmethod
    def backward(ctx, g):
        p, seed = ctx.meta
        g = _c(g)
        dx = torch.empty_like(g)
        call("hdmoe_dropout", dx, g, seed, step_counter(g.device), p, g.numel(), _dt(g))
        return dx, None, None


def dropout(x: Tensor, p: float, training: bool) -> Tensor:
    if not training or p == 0.0:
        return x
    return _DropoutFn.apply(x, float(p), _next_seed())


def randn_like(x: Tensor, scale) -> Tensor:
    """float32 normals of x's shape times `scale`, one value of the seed stream per call.  `scale`: a float, or a 1-element float32 device
    tensor that the kernel reads at run time -- the same values bit for bit, and a captured launch follows the tensor between replays."""
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if torch.is_tensor(scale):
        if scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != x.device:
            raise ValueError("randn_like: a tensor scale is one float32 element on x's device")
        call("hdmoe_randn_ds", out, _next_seed(), step_counter(x.device), scale, out.numel())
    else:
        call("hdmoe_randn", out, _next_seed(), step_counter(x.device), float(scale), out.numel())
    return out


def randn_keyed(x: Tensor, seed: int, stage: int) -> Tensor:
    """float32 standard normals of x's shape under the key (seed, stage): what hdmoe_randn writes for seed = `seed` and a device counter
    holding `stage`, i.e. the draw of the sampler's stochastic stage kernels.  Independent of the library's seed stream."""
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    key = (int(seed) + int(stage) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    call("hdmoe_randn", out, key, None, 1.0, out.numel())
    return out


def train_inputs(x: Tensor, sigma: Tensor, unet_mask: Tensor, vit_mask: Tensor, zeta_out: Tensor, src: Tensor, x0: Tensor,
                 unet_centers: Tensor, vit_centers: Tensor, seed: int, step: int, *, sigma_min: float, sigma_max: float, p_mean: float,
                 p_std: float, extreme_prob: float, unet_bw: float, vit_bw: float, min_active: int, zeta: float) -> None:
    """The inputs of training step `step` under `seed`, written into the caller's buffers in two launches (include/hdmoe.h,
    hdmoe_train_inputs: sigma (B,1,1,1), x = x0 + sigma eps, both router masks (B,E), zeta (1,), src (B,) int32).  Element j of eps is
    element j of randn_keyed(x, seed, 4 * step).  Nothing is read from torch's generator or the library's seed stream and nothing
    syncs.  ValueError -- before anything is written -- for B > 4096, E > 8, min_active > E, a non-contiguous or non-float32 tensor."""
    B = x0.shape[0] if x0.ndim else 0
    E = unet_centers.numel()
    want = {"x": (x, x0.shape, torch.float32), "sigma": (sigma, None, torch.float32), "unet_mask": (unet_mask, (B, E), torch.float32),
            "vit_mask": (vit_mask, (B, E), torch.float32), "zeta": (zeta_out, None, torch.float32), "src": (src, (B,), torch.int32),
            "x0": (x0, None, torch.float32), "unet_centers": (unet_centers, (E,), torch.float32), "vit_centers": (vit_centers, (E,), torch.float32)}
    for name, (t, shape, dt) in want.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"train_inputs: {name} must be contiguous {dt}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"train_inputs: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if B < 1 or sigma.numel() != B or zeta_out.numel() != 1 or int(step) < 0:
        raise ValueError("train_inputs: sigma holds B values, zeta one, step >= 0, B >= 1")
    try:
        call("hdmoe_train_inputs", x, sigma, unet_mask, vit_mask, zeta_out, src, x0, unet_centers, vit_centers,
             int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), B, x0.numel() // B, E, int(min_active), sigma_min, sigma_max, p_mean, p_std,
             extreme_prob, unet_bw, vit_bw, zeta)
    except RuntimeError as exc:
        if "invalid argument" in str(exc):                     # B > 4096, E > 8, min_active > E, a bad sigma range: nothing was launched
            raise ValueError(f"train_inputs: out of range (B={B} <= 4096, E={E} <= 8, min_active={min_active} <= E): {exc}") from None
        raise


def text_dropout(out: Tensor, keep: Tensor, text: Tensor, null: Optional[Tensor], seed: int, step: int, p: float) -> None:
    """Conditioning dropout of training step `step` under `seed` in one launch (include/hdmoe.h, hdmoe_text_dropout): keep (B,) float32
    0/1, out[i] = text[i] where keep[i] == 1 and `null` (one row, text.shape[1:]; None: zeros) otherwise.  text is (B, ...) float32,
    bfloat16 or float16; sample i is dropped iff its keyed draw is < float32(p).  Nothing is read from torch's generator or the library's
    seed stream and nothing syncs.  ValueError -- before anything is written -- for a non-contiguous tensor, out unlike text in dtype or
    shape, null not one row of text's dtype, keep not (B,) float32, out sharing storage with text, p outside [0, 1], step < 0."""
    if text.ndim < 2 or text.shape[0] < 1 or text.numel() == 0:
        raise ValueError(f"text_dropout: text is (B, ...) with B >= 1 and a non-empty row, got {tuple(text.shape)}")
    if text.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"text_dropout: text must be float32, bfloat16 or float16, got {text.dtype}")
    B = text.shape[0]
    want = {"out": (out, text.shape, text.dtype), "keep": (keep, (B,), torch.float32), "text": (text, None, text.dtype)}
    if null is not None:
        want["null"] = (null, text.shape[1:], text.dtype)
    for name, (t, shape, dt) in want.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"text_dropout: {name} must be contiguous {dt}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"text_dropout: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if out.is_cuda and text.is_cuda and out.untyped_storage().data_ptr() == text.untyped_storage().data_ptr():
        raise ValueError("text_dropout: out shares its storage with text")
    p = float(p)
    if not 0.0 <= p <= 1.0 or int(step) < 0:
        raise ValueError(f"text_dropout: p in [0, 1] and step >= 0, got p={p}, step={step}")
    call("hdmoe_text_dropout", out, keep, text, null, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), B, text.numel() // B,
         text.element_size(), p)


def dataset_inputs(x: Tensor, x0: Tensor, sigma: Tensor, unet_mask: Tensor, vit_mask: Tensor, zeta_out: Tensor, src: Tensor, item: Tensor,
                   flip: Tensor, mean: Tensor, std: Optional[Tensor], unet_centers: Tensor, vit_centers: Tensor, seed: int, data_seed: int,
                   step: int, *, world: int = 1, rank: int = 0, scale: float = 1.0, p_flip: float = 0.0, sigma_min: float, sigma_max: float,
                   p_mean: float, p_std: float, extreme_prob: float, unet_bw: float, vit_bw: float, min_active: int, zeta: float) -> None:
    """`train_inputs` with the latents made in the same call from a device-resident dataset (include/hdmoe.h, hdmoe_dataset_inputs):
    item (B,) int32 = the rows of `mean` / `std` (N,C,H,W), float32 or bfloat16, that step `step` holds for `rank` of `world` under
    `data_seed` (the seed before the rank is mixed in); flip (B,) float32 0/1; x0 (B,C,H,W) = scale * (mean + std * eps_p), mirrored
    along W where flip is 1 (`std` None: scale * mean); x = x0 + sigma eps.  Element j of eps_p is element j of
    randn_keyed(x, seed ^ 0xE7037ED1A0B428DB, 4 * step); sigma, eps, masks, zeta, src are train_inputs' for (seed, step).  Two launches, no
    sync.  ValueError -- before anything is written -- for what train_inputs rejects, a tensor of the wrong shape / dtype / layout,
    N < B * world, rank outside [0, world), p_flip outside [0, 1]."""
    if mean.ndim != 4 or mean.shape[0] < 1 or mean.numel() == 0:
        raise ValueError(f"dataset_inputs: mean is (N, C, H, W) with N >= 1, got {tuple(mean.shape)}")
    if mean.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dataset_inputs: mean must be float32 or bfloat16, got {mean.dtype}")
    if x0.ndim != 4 or tuple(x0.shape[1:]) != tuple(mean.shape[1:]) or x0.shape[0] < 1:
        raise ValueError(f"dataset_inputs: x0 has shape {tuple(x0.shape)}, expected (B,) + {tuple(mean.shape[1:])} with B >= 1")
    N, B, E = mean.shape[0], x0.shape[0], unet_centers.numel()
    want = {"x": (x, x0.shape, torch.float32), "x0": (x0, None, torch.float32), "sigma": (sigma, None, torch.float32),
            "unet_mask": (unet_mask, (B, E), torch.float32), "vit_mask": (vit_mask, (B, E), torch.float32), "zeta": (zeta_out, None, torch.float32),
            "src": (src, (B,), torch.int32), "item": (item, (B,), torch.int32), "flip": (flip, (B,), torch.float32),
            "mean": (mean, None, mean.dtype), "unet_centers": (unet_centers, (E,), torch.float32), "vit_centers": (vit_centers, (E,), torch.float32)}
    if std is not None:
        want["std"] = (std, mean.shape, mean.dtype)
    for name, (t, shape, dt) in want.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"dataset_inputs: {name} must be contiguous {dt}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"dataset_inputs: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if sigma.numel() != B or zeta_out.numel() != 1 or int(step) < 0:
        raise ValueError("dataset_inputs: sigma holds B values, zeta one, step >= 0")
    if x.untyped_storage().data_ptr() == x0.untyped_storage().data_ptr():
        raise ValueError("dataset_inputs: x shares its storage with x0")
    world, rank, p_flip, scale = int(world), int(rank), float(p_flip), float(scale)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"dataset_inputs: rank in [0, world) and world >= 1, got rank={rank}, world={world}")
    if N >= 1 << 31 or N < B * world:
        raise ValueError(f"dataset_inputs: N={N} items do not fill one step of B * world = {B} * {world} (and N < 2^31)")
    if not 0.0 <= p_flip <= 1.0 or scale != scale:
        raise ValueError(f"dataset_inputs: p_flip in [0, 1] and a scale that is a number, got p_flip={p_flip}, scale={scale}")
    M = 0xFFFFFFFFFFFFFFFF
    try:
        call("hdmoe_dataset_inputs", x, x0, sigma, unet_mask, vit_mask, zeta_out, src, item, flip, mean, std, _dt(mean), unet_centers,
             vit_centers, int(seed) & M, int(data_seed) & M, int(step), B, x0.numel() // B, N, mean.shape[2], mean.shape[3], world, rank,
             scale, p_flip, E, int(min_active), sigma_min, sigma_max, p_mean, p_std, extreme_prob, unet_bw, vit_bw, zeta)
    except RuntimeError as exc:
        if "invalid argument" in str(exc):                     # B > 4096, E > 8, min_active > E, a bad sigma range: nothing was launched
            raise ValueError(f"dataset_inputs: out of range (B={B} <= 4096, E={E} <= 8, min_active={min_active} <= E): {exc}") from None
        raise


def text_gather_dropout(out: Tensor, keep: Tensor, table: Tensor, text_index: Optional[Tensor], item: Tensor, null: Optional[Tensor],
                        seed: int, step: int, p: float, n_items: int) -> None:
    """`text_dropout` with row i of `out` (B, ...) taken from row t of `table` (K, ...): t = text_index[item[i]] with `text_index`
    (n_items,) int32, else 0 when K == 1 and item[i] when K == n_items (include/hdmoe.h, hdmoe_text_gather_dropout).  item (B,) int32
    holds dataset rows in [0, n_items) -- `dataset_inputs` writes it -- and `text_index` values in [0, K): neither is read back here, the
    caller has range-checked `text_index`.  keep and the drop decision are text_dropout's for (seed, step); p = 0 is a pure gather.
    ValueError -- before anything is written -- for a non-contiguous tensor, a wrong dtype or shape, K not in {1, n_items} without a
    text_index, out sharing storage with table, p outside [0, 1], step < 0."""
    if table.ndim < 2 or table.shape[0] < 1 or table.numel() == 0:
        raise ValueError(f"text_gather_dropout: table is (K, ...) with K >= 1 and a non-empty row, got {tuple(table.shape)}")
    if table.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"text_gather_dropout: table must be float32, bfloat16 or float16, got {table.dtype}")
    if item.ndim != 1 or item.shape[0] < 1:
        raise ValueError(f"text_gather_dropout: item is (B,) with B >= 1, got {tuple(item.shape)}")
    K, B, n_items = table.shape[0], item.shape[0], int(n_items)
    want = {"out": (out, (B,) + tuple(table.shape[1:]), table.dtype), "keep": (keep, (B,), torch.float32), "table": (table, None, table.dtype),
            "item": (item, None, torch.int32)}
    if null is not None:
        want["null"] = (null, table.shape[1:], table.dtype)
    if text_index is not None:
        want["text_index"] = (text_index, (n_items,), torch.int32)
    for name, (t, shape, dt) in want.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"text_gather_dropout: {name} must be contiguous {dt}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"text_gather_dropout: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if n_items < 1 or (text_index is None and K not in (1, n_items)):
        raise ValueError(f"text_gather_dropout: a table of K={K} rows for n_items={n_items} needs a text_index (K is neither 1 nor n_items)")
    if out.is_cuda and table.is_cuda and out.untyped_storage().data_ptr() == table.untyped_storage().data_ptr():
        raise ValueError("text_gather_dropout: out shares its storage with table")
    p = float(p)
    if not 0.0 <= p <= 1.0 or int(step) < 0:
        raise ValueError(f"text_gather_dropout: p in [0, 1] and step >= 0, got p={p}, step={step}")
    call("hdmoe_text_gather_dropout", out, keep, table, text_index, item, null, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), B, K, n_items,
         table.numel() // K, table.element_size(), p)


EVAL_SALT = 0x8EBC6AF09C88C6E3                                # the evaluation noise of include/hdmoe.h: randn_keyed(., seed ^ EVAL_SALT, item K + level)
EVAL_MAX_LEVELS, EVAL_MAX_BATCH, EVAL_MAX_EXPERTS = 64, 4096, 8


def eval_chunk() -> int:
    """Elements per fp32 partial sum of `eval_accumulate`'s first launch (hdmoe_eval_chunk)."""
    return int(lib().hdmoe_eval_chunk())


def eval_ws_floats(B: int, L: int) -> int:
    """float32 elements of the workspace `eval_accumulate` needs for a (B, L) batch."""
    c = eval_chunk()
    return int(B) * ((int(L) + c - 1) // c)


def eval_inputs(x: Tensor, x0: Tensor, sigma: Tensor, level: Tensor, item: Tensor, mean: Tensor, levels: Tensor, seed: int, round: int,
                first: int, count: int, *, scale: float = 1.0) -> None:
    """One held-out evaluation batch in one launch (include/hdmoe.h, hdmoe_eval_inputs): item[i] = (first + i) % N over the rows of
    `mean` (N, ...) float32 or bfloat16, level[i] = (item[i] + round) % K for i < count and -1 for the padding rows behind, sigma[i] =
    levels[(item[i] + round) % K] with `levels` (K,) float32, x0[i] = scale * mean[item[i]], x[i] = x0[i] + sigma[i] * eps where eps is
    randn_keyed(x[i], seed ^ EVAL_SALT, item[i] * K + level).  Nothing syncs.  ValueError -- before anything is written -- for a tensor of
    the wrong shape / dtype / layout, x sharing storage with x0, B > 4096, K > 64, count outside [0, B], a negative first or round."""
    if mean.ndim < 2 or mean.shape[0] < 1 or mean.numel() == 0:
        raise ValueError(f"eval_inputs: mean is (N, ...) with N >= 1 and a non-empty row, got {tuple(mean.shape)}")
    if mean.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"eval_inputs: mean must be float32 or bfloat16, got {mean.dtype}")
    if x0.ndim != mean.ndim or tuple(x0.shape[1:]) != tuple(mean.shape[1:]) or x0.shape[0] < 1:
        raise ValueError(f"eval_inputs: x0 has shape {tuple(x0.shape)}, expected (B,) + {tuple(mean.shape[1:])} with B >= 1")
    if levels.ndim != 1 or levels.numel() < 1:
        raise ValueError(f"eval_inputs: levels is (K,) with K >= 1, got {tuple(levels.shape)}")
    N, B, K = mean.shape[0], x0.shape[0], levels.numel()
    want = {"x": (x, x0.shape, torch.float32), "x0": (x0, None, torch.float32), "sigma": (sigma, None, torch.float32),
            "level": (level, (B,), torch.int32), "item": (item, (B,), torch.int32), "mean": (mean, None, mean.dtype),
            "levels": (levels, None, torch.float32)}
    for name, (t, shape, dt) in want.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"eval_inputs: {name} must be contiguous {dt}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"eval_inputs: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if sigma.numel() != B:
        raise ValueError("eval_inputs: sigma holds B values")
    if x.is_cuda and x0.is_cuda and x.untyped_storage().data_ptr() == x0.untyped_storage().data_ptr():
        raise ValueError("eval_inputs: x shares its storage with x0")
    round, first, count, scale = int(round), int(first), int(count), float(scale)
    if B > EVAL_MAX_BATCH or K > EVAL_MAX_LEVELS or N >= 1 << 31:
        raise ValueError(f"eval_inputs: out of range (B={B} <= {EVAL_MAX_BATCH}, K={K} <= {EVAL_MAX_LEVELS}, N={N} < 2^31)")
    if not 0 <= count <= B or first < 0 or round < 0 or scale != scale:
        raise ValueError(f"eval_inputs: count in [0, B], first >= 0, round >= 0 and a scale that is a number, got count={count}, "
                         f"first={first}, round={round}, scale={scale}")
    call("hdmoe_eval_inputs", x, x0, sigma, level, item, mean, _dt(mean), levels, int(seed) & 0xFFFFFFFFFFFFFFFF, round, first, count, B,
         x0.numel() // B, N, K, scale)


def eval_accumulate(acc: Tensor, ws: Tensor, denoised: Tensor, x0: Tensor, sigma: Tensor, level: Tensor, log_var: Optional[Tensor],
                    pU: Tensor, pV: Tensor, sigma_data: float) -> None:
    """acc (K, 6 + 4E) float64 += the per-level statistics of one batch, in two launches without atomics (include/hdmoe.h,
    hdmoe_eval_accumulate): row k = [n, sum mse, sum mse^2, sum w mse, sum (mse exp(-lv) + lv), sum lv, sum pU, #(pU > 0), sum pV,
    #(pV > 0)] over the samples with level == k.  denoised / x0 (B, ...) float32, sigma and log_var (None: lv = 0) B float32 values,
    level (B,) int32, pU / pV (B, E) float32, ws >= eval_ws_floats(B, L) float32.  The caller zeroes acc.  ValueError -- before
    anything is written -- for a tensor of the wrong shape / dtype / layout, B > 4096, E > 8, K > 64, a workspace that is too small."""
    if denoised.ndim < 2 or denoised.shape[0] < 1 or denoised.numel() == 0:
        raise ValueError(f"eval_accumulate: denoised is (B, ...) with B >= 1 and a non-empty row, got {tuple(denoised.shape)}")
    if pU.ndim != 2 or pU.shape[0] != denoised.shape[0] or pU.shape[1] < 1:
        raise ValueError(f"eval_accumulate: pU is (B, E) with E >= 1, got {tuple(pU.shape)}")
    B, E = pU.shape
    L = denoised.numel() // B
    if acc.ndim != 2 or acc.shape[0] < 1 or acc.shape[1] != 6 + 4 * E:
        raise ValueError(f"eval_accumulate: acc is (K, 6 + 4E) = (K, {6 + 4 * E}), got {tuple(acc.shape)}")
    K = acc.shape[0]
    want = {"acc": (acc, None, torch.float64), "ws": (ws, None, torch.float32), "denoised": (denoised, None, torch.float32),
            "x0": (x0, denoised.shape, torch.float32), "sigma": (sigma, None, torch.float32), "level": (level, (B,), torch.int32),
            "pU": (pU, None, torch.float32), "pV": (pV, (B, E), torch.float32)}
    if log_var is not None:
        want["log_var"] = (log_var, None, torch.float32)
    for name, (t, shape, dt) in want.items():
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"eval_accumulate: {name} must be contiguous {dt}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"eval_accumulate: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if sigma.numel() != B or (log_var is not None and log_var.numel() != B):
        raise ValueError("eval_accumulate: sigma and log_var hold B values")
    if B > EVAL_MAX_BATCH or E > EVAL_MAX_EXPERTS or K > EVAL_MAX_LEVELS:
        raise ValueError(f"eval_accumulate: out of range (B={B} <= {EVAL_MAX_BATCH}, E={E} <= {EVAL_MAX_EXPERTS}, K={K} <= {EVAL_MAX_LEVELS})")
    if ws.numel() < eval_ws_floats(B, L):
        raise ValueError(f"eval_accumulate: ws holds {ws.numel()} floats, a (B, L) = ({B}, {L}) batch needs {eval_ws_floats(B, L)}")
    call("hdmoe_eval_accumulate", acc, ws, denoised, x0, sigma, level, log_var, pU, pV, B, L, E, K, float(sigma_data))


# =====================================================================================================
# layout / boundary
# =====================================================================================================
class _ToNHWCFn(torch.autograd.Function):
    """float32 NCHW (contiguous) -> NHWC in `dtype`, optionally scaled per sample."""

    @staticmethod
    def forward(ctx, x, s, dtype):
        x = _c(x)
        N, C, H, W = x.shape
        out = torch.empty((N, H, W, C), dtype=dtype, device=x.device)
        call("hdmoe_nchw_to_nhwc", out, x, s, N, C, H * W, dtype_code(dtype))
        ctx.save_for_backward(s)
        return out

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        g = _c(g)
        N, H, W, C = g.shape
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
        call("hdmoe_nhwc_to_nchw", dx, g, s, None, None, N, C, H * W, _dt(g))
        return dx, None, None


class _FromNHWCFn(torch.autograd.Function):
    """out_nchw(fp32) = sf[n]*F_nhwc + sx[n]*x_nchw   (EDM D_x, model_config2.py:449)."""

    @staticmethod
    def forward(ctx, F, sf, x, sx):
        F = _c(F)
        N, H, W, C = F.shape
        x = None if x is None else _c(x)
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=F.device)
        call("hdmoe_nhwc_to_nchw", out, F, sf, x, sx, N, C, H * W, _dt(F))
        ctx.save_for_backward(sf, sx)
        ctx.meta = (F.dtype, x is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        sf, sx = ctx.saved_tensors
        fdt, has_x = ctx.meta
        g = _c(g)
        N, C, H, W = g.shape
        dF = torch.empty((N, H, W, C), dtype=fdt, device=g.device)
        call("hdmoe_nchw_to_nhwc", dF, g, sf, N, C, H * W, dtype_code(fdt))
        dx = None
        if has_x and ctx.needs_input_grad[2]:
            dx = torch.empty_like(g)
            if sx is None:
                call("hdmoe_axpby", dx, g, None, 1.0, 0.0, g.numel(), 0)
            else:
                call("hdmoe_scale_rows_fwd", dx, g, sx, N, C * H * W, 0)
        return dF, None, dx, None


def to_nhwc(x: Tensor, scale: Optional[Tensor] = None, dtype: Optional[torch.dtype] = None) -> Tensor:
    """Module-boundary ingest: logical NCHW -> contiguous (N,H,W,C)."""
    dtype = dtype or x.dtype
    if scale is None and dtype == x.dtype and x.is_contiguous(memory_format=torch.channels_last):
        return x.permute(0, 2, 3, 1)                      # already channel-last in memory: a view
    if x.dtype != torch.float32:
        # non-fp32 NCHW input at a module boundary: relayout only (no arithmetic)
        y = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        return cast(y, dtype) if scale is None else scale_rows(cast(y, dtype), scale)
    return _ToNHWCFn.apply(x, scale, dtype)


def from_nhwc(y: Tensor) -> Tensor:
    """(N,H,W,C) -> logical (N,C,H,W) (channels_last strides, zero-copy)."""
    return y.permute(0, 3, 1, 2)


def nhwc_to_nchw_f32(F: Tensor, sf: Optional[Tensor] = None, x: Optional[Tensor] = None, sx: Optional[Tensor] = None) -> Tensor:
    return _FromNHWCFn.apply(F, sf, x, sx)


def _row_scales(g: Tensor, rows: int, who: str) -> Tensor:
    """A per-sample guidance vector as the kernels read it: (rows,) float32, contiguous, on the GPU.  Its values are the caller's to check."""
    if g.dtype != torch.float32 or tuple(g.shape) != (rows,) or not g.is_cuda:
        raise ValueError(f"{who}: a guidance tensor must be a ({rows},) float32 CUDA tensor, got {tuple(g.shape)} {g.dtype} on {g.device}")
    return _c(g.detach())


def nhwc_to_nchw_guided(F: Tensor, sf: Tensor, x: Tensor, sx: Tensor, guidance: Union[float, Tensor]) -> Tensor:
    """Guided EDM egress of the pair-stacked head output F (2N, H, W, C) = [conditional ; unconditional]:
    out[n] = sx[n] x[n] + sf[n] ((1 - g) F[N + n] + g F[n]), float32 NCHW (N rows).  Inference only.
    guidance: a float, or a (N,) float32 CUDA tensor of per-sample scales g[n] (read on the device: nothing of it is baked into a capture)."""
    F = _c(F.detach())
    N2, H, W, C = F.shape
    if N2 % 2 or x.shape != (N2 // 2, C, H, W):
        raise ValueError(f"nhwc_to_nchw_guided: F {tuple(F.shape)} is not a pair-stacked batch of x {tuple(x.shape)}")
    N = N2 // 2
    g = _row_scales(guidance, N, "nhwc_to_nchw_guided") if isinstance(guidance, Tensor) else None
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=F.device)
    if g is None:
        call("hdmoe_nhwc_to_nchw_guided", out, F, _f32(sf.detach()), _f32(x.detach()), _f32(sx.detach()), float(guidance), N, C, H * W, _dt(F))
    else:
        call("hdmoe_nhwc_to_nchw_guided_rows", out, F, _f32(sf.detach()), _f32(x.detach()), _f32(sx.detach()), g, N, C, H * W, _dt(F))
    return out


def lerp_rows(ref: Tensor, d: Tensor, guidance: Union[float, Tensor]) -> Tensor:
    """The classifier-free-guidance blend (1 - g) ref + g d of two same-shaped (B, ...) tensors.  guidance: a float -- then this is
    axpby(ref, d, 1 - g, g) -- or a (B,) float32 CUDA tensor of per-sample scales, read on the device.  Inference only (no gradient)."""
    if not isinstance(guidance, Tensor):
        return axpby(ref, d, 1.0 - float(guidance), float(guidance))
    if ref.shape != d.shape or ref.dtype != d.dtype or ref.ndim < 1:
        raise ValueError(f"lerp_rows: ref {tuple(ref.shape)} {ref.dtype} and d {tuple(d.shape)} {d.dtype} differ")
    g = _row_scales(guidance, ref.shape[0], "lerp_rows")
    ref, d = _c(ref.detach()), _c(d.detach())
    out = torch.empty_like(ref)
    if ref.numel():
        call("hdmoe_lerp_rows", out, ref, d, g, ref.shape[0], ref.numel() // ref.shape[0], _dt(ref))
    return out


# Samples of at most this many elements stay in registers across the reduction of the guidance-combine kernel (every operand read once);
# larger ones re-read their operands after it.  HDMOE_GUIDE_COMBINE_RESIDENT of include/hdmoe.h.
GUIDE_COMBINE_RESIDENT = 16384


def _combine_args(who: str, guidance, rows: int, eta, norm_threshold, momentum, rescale, state, shape, device):
    """The launch scalars of the guidance combine as floats, the (rows,) scale vector or None, and the checked momentum buffer (None
    when momentum == 0: the kernel then neither reads nor writes one)."""
    eta, r, beta, phi = float(eta), float(norm_threshold), float(momentum), float(rescale)
    if not (0.0 <= eta <= 1.0 and r > 0.0 and -1.0 < beta < 1.0 and 0.0 <= phi <= 1.0):
        raise ValueError(f"{who}: needs eta in [0, 1], norm_threshold > 0, momentum in (-1, 1) and rescale in [0, 1], got eta={eta}, "
                         f"norm_threshold={r}, momentum={beta}, rescale={phi}")
    g = _row_scales(guidance, rows, who) if isinstance(guidance, Tensor) else None
    if g is None and not math.isfinite(float(guidance)):
        raise ValueError(f"{who}: guidance must be finite, got {guidance}")
    if beta == 0.0:
        return eta, r, beta, phi, g, None
    if not isinstance(state, Tensor) or state.dtype != torch.float32 or tuple(state.shape) != tuple(shape) or state.device != device \
            or not state.is_contiguous():
        raise ValueError(f"{who}: momentum != 0 needs state, a contiguous float32 tensor of shape {tuple(shape)} on {device} (the momentum "
                         f"buffer, updated in place), got {type(state).__name__ if not isinstance(state, Tensor) else (tuple(state.shape), state.dtype, state.device)}")
    return eta, r, beta, phi, g, state


def guide_combine(ref: Tensor, d: Tensor, guidance: Union[float, Tensor], *, eta: float = 1.0, norm_threshold: float = float("inf"),
                  momentum: float = 0.0, rescale: float = 0.0, state: Optional[Tensor] = None) -> Tensor:
    """Guidance rescale and adaptive projected guidance (APG) of the two-pass outputs ref = D_u and d = D_c, same-shaped (B, ...), in one
    launch; every sum runs over one sample (hdmoe_guide_combine, include/hdmoe.h, has the formulas):
      M = (D_c - D_u) + momentum * state (state <- M, float32, in place; momentum == 0: no state is read or written),
      out = f (a D_c + b M): b = (w - 1) min(1, norm_threshold / |M|), a = 1 - b (1 - eta) <M, D_c> / |D_c|^2,
      f = rescale * std(D_c) / std(a D_c + b M) + 1 - rescale.
    guidance: w, a float, or a (B,) float32 CUDA tensor read on the device.  eta = 1, norm_threshold = inf, momentum = 0, rescale = 0 is
    (1 - w) D_u + w D_c.  Inference only (no gradient)."""
    if ref.shape != d.shape or ref.dtype != d.dtype or ref.ndim < 1 or ref.numel() == 0:
        raise ValueError(f"guide_combine: ref {tuple(ref.shape)} {ref.dtype} and d {tuple(d.shape)} {d.dtype} differ (or are empty)")
    rows = ref.shape[0]
    eta, r, beta, phi, g, state = _combine_args("guide_combine", guidance, rows, eta, norm_threshold, momentum, rescale, state, ref.shape,
                                                ref.device)
    ref, d = _c(ref.detach()), _c(d.detach())
    out = torch.empty_like(ref)
    call("hdmoe_guide_combine", out, ref, d, 0.0 if g is not None else float(guidance), g, eta, r, beta, phi, state, rows,
         ref.numel() // rows, _dt(ref))
    return out


def nhwc_to_nchw_guide_combine(F: Tensor, sf: Tensor, x: Tensor, sx: Tensor, guidance: Union[float, Tensor], *, eta: float = 1.0,
                               norm_threshold: float = float("inf"), momentum: float = 0.0, rescale: float = 0.0,
                               state: Optional[Tensor] = None) -> Tensor:
    """guide_combine as the egress of the pair-stacked head output F (2N, H, W, C) = [conditional ; unconditional]: D_c = sx[n] x[n] +
    sf[n] F[n] and D_u = sx[n] x[n] + sf[n] F[N + n] are formed in registers, the result is float32 NCHW (N rows); state (momentum != 0):
    (N, C, H, W) float32.  Inference only."""
    F = _c(F.detach())
    N2, H, W, C = F.shape
    if N2 % 2 or x.shape != (N2 // 2, C, H, W):
        raise ValueError(f"nhwc_to_nchw_guide_combine: F {tuple(F.shape)} is not a pair-stacked batch of x {tuple(x.shape)}")
    N = N2 // 2
    eta, r, beta, phi, g, state = _combine_args("nhwc_to_nchw_guide_combine", guidance, N, eta, norm_threshold, momentum, rescale, state,
                                                (N, C, H, W), F.device)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=F.device)
    call("hdmoe_nhwc_to_nchw_guide_combine", out, F, _f32(sf.detach()), _f32(x.detach()), _f32(sx.detach()),
         0.0 if g is not None else float(guidance), g, eta, r, beta, phi, state, N, C, H * W, _dt(F))
    return out


# At most this many conditions in one composed evaluation.  HDMOE_COMPOSE_MAX of include/hdmoe.h.
COMPOSE_MAX = 8


def _compose_args(who: str, weights, masks, rows: int, K: int, spatial, device):
    """The weights (rows, K) and masks (rows, K, *spatial) or None of a composed evaluation as the kernels read them: float32, contiguous,
    on `device`.  Their values are the caller's to check (nothing is read from the device here)."""
    if not 1 <= K <= COMPOSE_MAX:
        raise ValueError(f"{who}: needs 1 <= K <= {COMPOSE_MAX} conditions, got {K}")
    if not isinstance(weights, Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (rows, K) or weights.device != device:
        raise ValueError(f"{who}: weights must be a ({rows}, {K}) float32 tensor on {device}, got "
                         f"{(tuple(weights.shape), weights.dtype, weights.device) if isinstance(weights, Tensor) else type(weights).__name__}")
    if masks is not None:
        want = (rows, K) + tuple(spatial)
        if not isinstance(masks, Tensor) or masks.dtype != torch.float32 or tuple(masks.shape) != want or masks.device != device:
            raise ValueError(f"{who}: masks must be None or a {want} float32 tensor on {device}, got "
                             f"{(tuple(masks.shape), masks.dtype, masks.device) if isinstance(masks, Tensor) else type(masks).__name__}")
        masks = _c(masks.detach())
    return _c(weights.detach()), masks


def guide_compose(ref: Tensor, ds: Sequence[Tensor], weights: Tensor, masks: Optional[Tensor], guidance: Union[float, Tensor], *,
                  eta: float = 1.0, norm_threshold: float = float("inf"), momentum: float = 0.0, rescale: float = 0.0,
                  state: Optional[Tensor] = None) -> Tensor:
    """Composed guidance of the two-pass outputs: ref = D_u and ds = [D_1, ..., D_K], all (B, C, *spatial) of one dtype, become
    D_c = D_u + sum_k c_k (D_k - D_u), c_k = weights[n, k] * masks[n, k, p] (masks None: c_k = weights[n, k]), formed in registers in front
    of the steps of guide_combine, in one launch (hdmoe_guide_compose, include/hdmoe.h, has the arithmetic).  weights: (B, K) float32;
    masks: None or (B, K, *spatial) float32 in [0, 1], broadcast over channels.  K = 1, weights 1, no masks is guide_combine(ref, ds[0])
    bit for bit; guidance 1 with the default scalars returns D_c.  Inference only (no gradient)."""
    ds = list(ds)
    K = len(ds)
    if ref.ndim < 1 or ref.numel() == 0 or any(not isinstance(d, Tensor) or d.shape != ref.shape or d.dtype != ref.dtype or
                                               d.device != ref.device for d in ds):
        raise ValueError(f"guide_compose: every entry of ds must be a tensor like ref {tuple(ref.shape)} {ref.dtype} (and ref not empty)")
    rows = ref.shape[0]
    a, m = _compose_args("guide_compose", weights, masks, rows, K, ref.shape[2:], ref.device)
    eta, r, beta, phi, g, state = _combine_args("guide_compose", guidance, rows, eta, norm_threshold, momentum, rescale, state, ref.shape,
                                                ref.device)
    ref, ds = _c(ref.detach()), [_c(d.detach()) for d in ds]
    out = torch.empty_like(ref)
    hw = 1
    for s in ref.shape[2:]:
        hw *= s
    call("hdmoe_guide_compose", out, ref, ds, K, a, m, hw, 0.0 if g is not None else float(guidance), g, eta, r, beta, phi, state, rows,
         ref.numel() // rows, _dt(ref))
    return out


def nhwc_to_nchw_compose(F: Tensor, sf: Tensor, x: Tensor, sx: Tensor, K: int, weights: Tensor, masks: Optional[Tensor],
                         guidance: Union[float, Tensor], *, eta: float = 1.0, norm_threshold: float = float("inf"), momentum: float = 0.0,
                         rescale: float = 0.0, state: Optional[Tensor] = None) -> Tensor:
    """guide_compose as the egress of the variant-stacked head output F ((K + 1) N, H, W, C): rows k N .. k N + N - 1 belong to condition
    k + 1, the last N rows are unconditional.  D_k = sx[n] x[n] + sf[n] F[k N + n] and D_u are formed in registers; the result is float32
    NCHW (N rows).  weights (N, K), masks None or (N, K, H, W), state (momentum != 0): (N, C, H, W) float32.  Inference only."""
    F = _c(F.detach())
    NV, H, W, C = F.shape
    K = int(K)
    if not 1 <= K <= COMPOSE_MAX:
        raise ValueError(f"nhwc_to_nchw_compose: needs 1 <= K <= {COMPOSE_MAX} conditions, got {K}")
    if NV % (K + 1) or x.shape != (NV // (K + 1), C, H, W):
        raise ValueError(f"nhwc_to_nchw_compose: F {tuple(F.shape)} is not a batch of x {tuple(x.shape)} stacked {K + 1} times")
    N = NV // (K + 1)
    a, m = _compose_args("nhwc_to_nchw_compose", weights, masks, N, K, (H, W), F.device)
    eta, r, beta, phi, g, state = _combine_args("nhwc_to_nchw_compose", guidance, N, eta, norm_threshold, momentum, rescale, state,
                                                (N, C, H, W), F.device)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=F.device)
    call("hdmoe_nhwc_to_nchw_compose", out, F, _f32(sf.detach()), _f32(x.detach()), _f32(sx.detach()), K, a, m,
         0.0 if g is not None else float(guidance), g, eta, r, beta, phi, state, N, C, H * W, _dt(F))
    return out


class _PatchRelayoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, meta):
        N, H, W, C, p, hp, wp, order = meta
        tok = _c(tok)
        out = torch.empty((N, H, W, C), dtype=tok.dtype, device=tok.device)
        _call_or("hdmoe_patch_relayout_tiled", "hdmoe_patch_relayout", out, tok, N, H, W, C, p, hp, wp, order, 1, _dt(tok))
        ctx.meta = meta
        ctx.tshape = tok.shape
        return out

    @staticmethod
    def backward(ctx, g):
        N, H, W, C, p, hp, wp, order = ctx.meta
        g = _c(g)
        # tokens cover the padded hp*p x wp*p canvas; positions outside H x W receive no gradient
        dtok = torch.zeros(ctx.tshape, dtype=g.dtype, device=g.device) if (hp * p != H or wp * p != W) else \
            torch.empty(ctx.tshape, dtype=g.dtype, device=g.device)
        _call_or("hdmoe_patch_relayout_tiled", "hdmoe_patch_relayout", dtok, g, N, H, W, C, p, hp, wp, order, 0, _dt(g))
        return dtok, None


def pixel_shuffle_tokens(tok: Tensor, H: int, W: int, C: int, p: int) -> Tensor:
    """tokens (N, hp*wp, C*p*p) in PixelShuffle feature order -> image (N,H,W,C), cropped (model_components.py:698-704)."""
    N = tok.shape[0]
    hp, wp = -(-H // p), -(-W // p)
    return _PatchRelayoutFn.apply(tok, (N, H, W, C, p, hp, wp, 1))


# =====================================================================================================
# norms
# =====================================================================================================
class _PixelNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, with_silu, gx_scale=1.0):
        ctx.sx = float(gx_scale)
        x = _c(x)
        C = x.shape[-1]
        xn = torch.empty_like(x)
        h = torch.empty_like(x) if with_silu else None
        call("hdmoe_pixelnorm_fwd", xn, h, x, x.numel() // C, C, _dt(x))
        ctx.save_for_backward(x)
        ctx.with_silu = with_silu
        if with_silu:
            return xn, h
        return xn

    @staticmethod
    def backward(ctx, dxn, dh=None):
        (x,) = ctx.saved_tensors
        C = x.shape[-1]
        dx = torch.empty_like(x)
        call("hdmoe_pixelnorm_bwd", dx, _c(dxn), _c(dh), x, x.numel() // C, C, ctx.sx, _dt(x))
        return dx, None, None


def pixel_norm(x: Tensor) -> Tensor:
    """normalize(x, dim=[channel]) (model_internals.py:8-30)."""
    return _PixelNormFn.apply(x, False, 1.0)


def pixel_norm_silu(x: Tensor, gx_scale: float = 1.0):
    """Returns (normalize(x, channel), mp_silu(of that)) in one pass (model_components.py:238-240).  ``gx_scale``: factor applied to
    the gradient arriving for the FIRST output (see mp_conv(res_grad_raw=True))."""
    return _PixelNormFn.apply(x, True, float(gx_scale))


class _GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, G, act, eps):
        x = _c(x)
        N, C = x.shape[0], x.shape[-1]
        S = x.numel() // (N * C)
        mean = torch.empty(N * G, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        y = torch.empty_like(x)
        parts = _gn_parts(N, S)
        if parts > 1:
            ws = torch.empty(2 * N * parts * G, dtype=torch.float32, device=x.device)
            call("hdmoe_groupnorm_fwd_split", y, mean, rstd, ws, parts, x, gamma, beta, N, S, C, G, act, eps, _dt(x))
        else:
            call("hdmoe_groupnorm_fwd", y, mean, rstd, x, gamma, beta, N, S, C, G, act, eps, _dt(x))
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.meta = (N, S, C, G, act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        N, S, C, G, act = ctx.meta
        g = _c(g)
        dx = torch.empty_like(x)
        direct = _direct(gamma) and _direct(beta)
        dgamma = gamma.grad if direct else torch.zeros_like(gamma)
        dbeta = beta.grad if direct else torch.zeros_like(beta)
        parts = _gn_parts(N, S, forward=False)
        if parts > 1:
            ws = _zeros((2 * N * G,), torch.float32, x.device)
            call("hdmoe_groupnorm_bwd_split", dx, dgamma, dbeta, ws, parts, g, x, gamma, beta, mean, rstd, N, S, C, G, act, _dt(x))
        else:
            ws = torch.empty(2 * N * G, dtype=torch.float32, device=x.device)
            call("hdmoe_groupnorm_bwd", dx, dgamma, dbeta, ws, g, x, gamma, beta, mean, rstd, N, S, C, G, act, _dt(x))
        if direct:
            return dx, None, None, None, None, None
        return dx, dgamma, dbeta, None, None, None


def _gn_parts(N: int, S: int, forward: bool = True) -> int:
    """Row-range workgroups per sample for the GroupNorm statistics.  Forward: a function of S only -- the summation order, and
    with it every bit of the output, must not depend on how many samples share the batch.  Backward (which sums with float
    atomics anyway): only when one block per sample would leave the chip idle."""
    if forward:
        return max(1, min(4, S // 256))
    if N >= 128 or S < 256:
        return 1
    return max(1, min(64, 256 // N, S // 128))


ACT_NONE, ACT_RELU, ACT_MP_SILU = 0, 1, 2


def group_norm(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, act: int = ACT_NONE, eps: float = 1e-5) -> Tensor:
    """nn.GroupNorm over a channel-last tensor (N, ..., C), optionally fused with ReLU / mp_silu."""
    return _GroupNormFn.apply(x, gamma, beta, int(groups), int(act), float(eps))


TRUNK_FUSED = True
# bf16 compute mode only (the split kernels): the router trunks' BACKWARD (input + weight gradients of their convs) uses the hi halves of
# the split operands only -- bf16 operands, fp32 accumulation, one MFMA per product instead of three.  Bit-exact routing indices need
# the fp32-equivalent FORWARD (three products); gradients carry the bf16 mode's tolerance like every expert layer.  False: three products.
TRUNK_BWD_BF16 = True


class _TrunkFn(torch.autograd.Function):
    """Router.hard_route up to the average pool (reference model_components.py:100-112): three [MP_Conv 3x3 -> GroupNorm(1, C) -> ReLU]
    and AdaptiveAvgPool2d(1) over an fp32 channel-last tensor, with the GroupNorm + ReLU folded into the convs on either side
    (split-bf16 arithmetic, csrc/conv6s.hip):
      conv_l writes y_l and per-sample partial statistics of y_l -> hdmoe_gn1_finalize -> scale_l / shift_l [N][C];
      conv_{l+1} (and, in the backward, its weight gradient) stage relu(y_l * scale_l + shift_l) instead of a stored activation;
      the last GroupNorm + ReLU + pool is one read of y_3 (hdmoe_gn1_relu_mean).
    The normalised activations are never written.  ``tensors`` = (weight, gamma, beta) x 3; ``ents`` the ready weight-bank entries."""

    @staticmethod
    def forward(ctx, x, ents, bank, eps, grad, *tensors):
        x = _c(x)
        N, H, W, _ = x.shape
        S = H * W
        inp, sc, sh = x, None, None
        saved = []
        # the backward takes the bf16 streaming path: the last layer's backward sums then come from two (N, C) statistics of this forward.
        # `grad`: grad mode was on at the call and something requires a gradient (inside forward() grad mode is always off, and
        # ctx.needs_input_grad says nothing about a no_grad caller)
        pq = (None, None)
        if grad and _trunk_use7(N, H, W, tensors):
            C3 = int(tensors[6].shape[0])
            pq = (torch.empty((N, C3), dtype=torch.float32, device=x.device), torch.empty((N, C3), dtype=torch.float32, device=x.device))
        for l in range(3):
            w, gamma, beta = tensors[3 * l:3 * l + 3]
            O, I = int(w.shape[0]), int(w.shape[1])
            ent = ents[l]
            slots = lib().hdmoe_conv_split_stats_slots(H, W, O)
            y = torch.empty((N, H, W, O), dtype=torch.float32, device=x.device)
            ws = torch.empty((N, max(slots, 1), 2), dtype=torch.float32, device=x.device)
            if slots < 1 or _timed("fused", dict(name=f"conv6_split_kernel<{2 if O % 64 == 0 else 1}> (GroupNorm folded)", dtype="split_bf16", seg=None, N=N, HW=S, O=O, I=I, taps=[9], mult=1.0),
                                   "hdmoe_conv_fwd_split_gn", inp, ent.wf, y, sc, sh, 1, ws, ent.wstride, ent.wstride, N, H, W, I, O, 1.0) != 0:
                raise RuntimeError("router trunk: layer outside the split conv kernel's domain (ops.trunk_ok should have said so)")
            sc = torch.empty((N, O), dtype=torch.float32, device=x.device)
            sh = torch.empty_like(sc)
            mean = torch.empty(N, dtype=torch.float32, device=x.device)
            rstd = torch.empty_like(mean)
            if l < 2:
                # (folding this step into the consuming conv as well -- every workgroup re-deriving mean / rstd from the slots in fp64 --
                #  was measured 0.08 ms/step SLOWER: register spills in the 128-channel kernel; tried and removed)
                call("hdmoe_gn1_finalize", sc, sh, mean, rstd, ws, gamma, beta, N, slots, O, S * O, eps[l])
            else:                                               # last layer: statistics -> scale / shift inside the pooled read's launch
                out = torch.empty((N, O), dtype=torch.float32, device=x.device)
                if pq[0] is not None:
                    call("hdmoe_gn1_finalize_relu_mean_pq", out, sc, sh, mean, rstd, *pq, y, ws, gamma, beta, N, slots, S, O, eps[l])
                else:
                    call("hdmoe_gn1_finalize_relu_mean", out, sc, sh, mean, rstd, y, ws, gamma, beta, N, slots, S, O, eps[l])
            saved += [y, sc, sh, mean, rstd]
            inp = y
        ctx.save_for_backward(x, *saved, *pq, *tensors)
        ctx.ents, ctx.bank = ents, bank
        STATS["trunk"] += 1
        return out

    @staticmethod
    def backward(ctx, g):
        x, *rest = ctx.saved_tensors
        saved, (pcnt, qsum), tensors = rest[:15], rest[15:17], rest[17:]
        N, H, W, _ = x.shape
        S = H * W
        ents, bank = ctx.ents, ctx.bank
        params = [t for l in range(3) for t in tensors[3 * l + 1:3 * l + 3]]
        bufs, ret = _param_grads(params)
        da = None
        # bf16-operand mode on 32 x 32 maps with enough samples: the trunk backward as PLAIN bf16 layers on the streaming kernels (csrc/conv7_body.h,
        # wgrad7_body.h) -- the GroupNorm backward writes dy_l in bf16 and, in the same launch, materialises the conv input relu(gn(y_{l-1}))
        # in bf16 (the forward never stores it), and the fused dgrad + weight-gradient launch reads both by LDS-DMA.  Same arithmetic as the hi-only
        # split path (bf16 operands, fp32 accumulation) except that the input gradient between two layers is stored in bf16.
        use7 = _trunk_use7(N, H, W, tensors)
        assert not use7 or pcnt is not None
        for l in (2, 1, 0):
            w, gamma, beta = tensors[3 * l:3 * l + 3]
            y, sc, sh, mean, rstd = saved[5 * l:5 * l + 5]
            O, I = int(w.shape[0]), int(w.shape[1])
            ent = ents[l]
            xin = x if l == 0 else saved[5 * (l - 1)]
            isc, ish = (None, None) if l == 0 else (saved[5 * (l - 1) + 1], saved[5 * (l - 1) + 2])
            if use7:
                # GroupNorm + ReLU backward -> dy_l and relu(gn(y_{l-1})) -> the conv input, both bf16, in one launch (csrc/norm.hip
                # gn1t_apply_kernel); its sums come from a statistics launch over (y_l, da), or for the pooled last layer from the forward's
                # pcnt / qsum -- fixed summation orders, no float atomics
                dyb = torch.empty(y.shape, dtype=torch.bfloat16, device=x.device)
                a_in = torch.empty(xin.shape, dtype=torch.bfloat16, device=x.device)
                stw = None
                if l < 2:
                    stw = torch.empty(lib().hdmoe_gn1t_stats_floats(N, S, O), dtype=torch.float32, device=x.device)
                    call("hdmoe_gn1t_stats", stw, da, y, gamma, beta, mean, rstd, N, S, O)
                call("hdmoe_gn1t_apply", dyb, a_in, bufs[2 * l], bufs[2 * l + 1], stw, None if l == 2 else da, _f32(g) if l == 2 else None,
                     1.0 / S if l == 2 else 1.0, pcnt if l == 2 else None, qsum if l == 2 else None, y, gamma, beta, mean, rstd,
                     xin, isc, ish, N, S, O, I)
                L = _ConvLayer.of_entry(ent, N, H, W, BF16)
                plan = _kxk_bwd_plan(L, None, "own", ("trunk_bwd", "trunk_bwd7"), "bwd7_trunk_kernel")
                arena = plan.workspace(L, x.device)
                da = torch.empty(xin.shape, dtype=torch.bfloat16, device=x.device)
                if not plan.launch(bank, ent, a_in, dyb, da, arena):
                    raise RuntimeError("router trunk backward: layer outside the streaming backward kernels' domain")
                if l == 0:                                     # the stem features are fp32: so is their gradient
                    da32 = torch.empty(xin.shape, dtype=torch.float32, device=x.device)
                    call("hdmoe_cast", da32, da, da.numel(), 1, 0)
                    da = da32
                continue
            dy = torch.empty_like(y)
            ws = torch.empty(2 * N, dtype=torch.float32, device=x.device)
            if l == 2:      # d(mean over S of a_3): g[n][c] / S at every position, read from the (N, C) tensor (no materialised broadcast)
                call("hdmoe_groupnorm_bwd_bcast", dy, bufs[2 * l], bufs[2 * l + 1], ws, _f32(g), 1.0 / S, y, gamma, beta, mean, rstd, N, S, O, 1, ACT_RELU, 0)
            else:
                call("hdmoe_groupnorm_bwd", dy, bufs[2 * l], bufs[2 * l + 1], ws, da, y, gamma, beta, mean, rstd, N, S, O, 1, ACT_RELU, 0)
            L = _ConvLayer.of_entry(ent, N, H, W, F32S)
            plan = _kxk_bwd_plan(L, None, "own", ("trunk_bwd",), "bwd6s_kernel", gn_in=(isc, ish, 1))
            arena = plan.workspace(L, x.device)
            da = torch.empty_like(xin)
            if not plan.launch(bank, ent, xin, dy, da, arena):
                raise RuntimeError("router trunk backward: layer outside the fused backward kernel's domain")
        out = [da, None, None, None, None]
        for l in range(3):
            out += [None, ret[2 * l], ret[2 * l + 1]]
        return tuple(out)


def _trunk_use7(N: int, H: int, W: int, tensors) -> bool:
    """Does _TrunkFn's backward run as plain bf16 layers on the streaming kernels (32 x 32 maps, enough samples, widths % 32)?"""
    return (TRUNK_BWD_BF16 and H == 32 and W == 32 and N >= _c7_min_images()
            and all(int(tensors[3 * l].shape[0]) % 32 == 0 and int(tensors[3 * l].shape[1]) % 32 == 0 for l in range(3)))


def trunk_ok(x: Tensor, convs) -> bool:
    """Can Router.hard_route take the fused path?  bf16 compute mode with split-bf16 trunks, every conv a ready weight-bank entry inside the
    split kernels' domain, and the deferred weight-gradient path on."""
    if not (TRUNK_FUSED and _prof_ok() and _bank.ACTIVE is not None):
        return False
    if x.dtype != torch.float32 or x.ndim != 4:
        return False
    c = x.shape[-1]
    for w in convs:
        if int(w.shape[1]) != c or not _split_ok(*x.shape[:3], c, [w]):
            return False
        c = int(w.shape[0])
        # every layer's GroupNorm backward runs on the 16-byte-vector kernels only (the pooled-gradient form hdmoe_groupnorm_bwd_bcast has no
        # scalar fallback): csrc/norm.hip gn_vec_ok -- C / 4 lanes per pixel must divide the 512-thread block
        cv = c // 4
        if c % 4 or cv > 512 or 512 % cv:
            return False
    return c <= 1024                                         # hdmoe_gn1_finalize_relu_mean: one pixel row of <= 1024 channels per pass


def router_trunk(x: Tensor, convs, norms) -> Optional[Tensor]:
    """Fused Router.hard_route[0:10] -> (N, 4C) fp32, or None when the weight bank has not prepared the layers yet (the caller then
    runs the layers one by one; the lookup registers them for the next step)."""
    ents = [_bank.ACTIVE.lookup([w], "split", 1.0, 1.0, True) for w in convs]
    if any(e is None for e in ents):
        return None
    tensors = []
    for w, nm in zip(convs, norms):
        tensors += [w, nm.weight, nm.bias]
    grad = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in tensors))
    return _TrunkFn.apply(x, ents, _bank.ACTIVE, [float(nm.eps) for nm in norms], grad, *tensors)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = _c(x)
        C = x.shape[-1]
        rows = x.numel() // C
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        y = torch.empty_like(x)
        call("hdmoe_layernorm_fwd", y, mean, rstd, x, gamma, beta, rows, C, eps, _dt(x))
        ctx.save_for_backward(x, gamma, mean, rstd, beta)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, rstd, beta = ctx.saved_tensors
        g = _c(g)
        C = x.shape[-1]
        dx = torch.empty_like(x)
        direct = _direct(gamma) and _direct(beta)
        dgamma = gamma.grad if direct else torch.zeros_like(gamma)
        dbeta = beta.grad if direct else torch.zeros_like(gamma)
        call("hdmoe_layernorm_bwd", dx, dgamma, dbeta, g, x, gamma, mean, rstd, x.numel() // C, C, _dt(x))
        if direct:
            return dx, None, None, None
        return dx, dgamma, dbeta, None


def layer_norm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5) -> Tensor:
    return _LayerNormFn.apply(x, gamma, beta, float(eps))


# =====================================================================================================
# attention core
# =====================================================================================================
class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, bias, H):
        q = _c(q); k = _c(k); v = _c(v)
        B, Sq, E = q.shape
        Skv = k.shape[1]
        D = E // H
        Sb = 0
        if bias is not None:
            bias = _f32(bias)
            Sb = bias.shape[-1]
        out = torch.empty_like(q)
        lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
        _timed("attn", dict(dir="fwd", B=B, Sq=Sq, Skv=Skv, H=H, D=D, esz=q.element_size(), bias=bias is not None),
               "hdmoe_attn_fwd", out, lse, q, k, v, bias, B, Sq, Skv, H, D, Sb, _dt(q))
        ctx.save_for_backward(q, k, v, bias, out, lse)
        ctx.H = H
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, bias, out, lse = ctx.saved_tensors
        H = ctx.H
        g = _c(g)
        B, Sq, E = q.shape
        Skv = k.shape[1]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        dbias = None
        Sb = 0
        direct = False
        if bias is not None:
            Sb = bias.shape[-1]
            if ctx.needs_input_grad[3]:
                direct = _direct(bias)
                dbias = bias.grad if direct else torch.zeros_like(bias)
        _timed("attn", dict(dir="bwd", B=B, Sq=Sq, Skv=Skv, H=H, D=E // H, esz=q.element_size(), bias=bias is not None),
               "hdmoe_attn_bwd", dq, dk, dv, dbias, delta, g, out, q, k, v, lse, bias, B, Sq, Skv, H, E // H, Sb, _dt(q))
        return dq, dk, dv, (None if direct else dbias), None


class _BicubicFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, S):
        table = _f32(table)
        H, S0, _ = table.shape
        out = torch.empty((H, S, S), dtype=torch.float32, device=table.device)
        call("hdmoe_bicubic_fwd", out, table, H, S0, S)
        ctx.dims = (H, S0, S)
        return out

    @staticmethod
    def backward(ctx, g):
        H, S0, S = ctx.dims
        dt = torch.zeros((H, S0, S0), dtype=torch.float32, device=g.device)
        call("hdmoe_bicubic_bwd", dt, _f32(g), H, S0, S)
        return dt, None


def bicubic_resize(table: Tensor, S: int) -> Tensor:
    """(H,S0,S0) -> (H,S,S): F.interpolate(mode='bicubic', align_corners=False) of the rel_pos_bias table
    (reference model_internals.py:388-397)."""
    return _BicubicFn.apply(table, int(S))


def attention(q: Tensor, k: Tensor, v: Tensor, bias: Optional[Tensor], num_heads: int) -> Tensor:
    """softmax(q k^T / sqrt(D) + bias) v per head; (B,S,E) tensors, head h = channels [h*D,(h+1)*D)."""
    return _AttnFn.apply(q, k, v, bias, int(num_heads))


# =====================================================================================================
# ragged tokens: the ViT expert bank (csrc/ragged.hip, hdmoe_attn_rag_* in csrc/attention.hip)
# =====================================================================================================
class RagLayout:
    """Routed rows of all ViT experts in one padded tensor (R, Sp, C): rows [seg[g], seg[g+1]) (device int32, from the
    dispatch plan) belong to expert g and hold ``lens[g]`` real tokens followed by padding."""

    def __init__(self, seg: Tensor, lens: Sequence[int], R: int):
        self.seg, self.lens, self.R = seg, [int(v) for v in lens], int(R)
        self.G, self.Sp = len(self.lens), max(int(v) for v in lens)


def _param_grads(params):
    """(buffers the kernels accumulate into, what to hand back to autograd) for small fp32 parameters."""
    direct = all(_direct(p) for p in params)
    bufs = [p.grad if direct else torch.zeros_like(p) for p in params]
    return bufs, ([None] * len(params) if direct else bufs)


class _RagPackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rag, *tensors):
        G = rag.G
        srcs, pos = [_c(t) for t in tensors[:G]], tensors[G:]
        C = srcs[0].shape[-1]
        dst = torch.empty((rag.R, rag.Sp, C), dtype=srcs[0].dtype, device=srcs[0].device)
        call("hdmoe_rag_pack", dst, srcs, [_f32(p) for p in pos], rag.seg, rag.lens, G, rag.R, rag.Sp, C, _dt(dst))
        ctx.rag, ctx.C = rag, C
        ctx.save_for_backward(*pos)
        return dst

    @staticmethod
    def backward(ctx, g):
        rag, C, pos = ctx.rag, ctx.C, ctx.saved_tensors
        g = _c(g)
        dsrcs = [torch.empty((rag.R, L, C), dtype=g.dtype, device=g.device) for L in rag.lens]
        bufs, ret = _param_grads(pos)
        call("hdmoe_rag_pack_bwd", dsrcs, bufs, g, rag.seg, rag.lens, rag.G, rag.R, rag.Sp, C, _dt(g))
        return (None, *dsrcs, *ret)


def rag_pack(srcs: Sequence[Tensor], pos: Sequence[Tensor], rag: RagLayout) -> Tensor:
    """Per-expert compact tokens (R, S_g, C) (+ that expert's pos_emb (1, S_g, C)) -> padded (R, Sp, C); row r takes expert g(r)'s."""
    return _RagPackFn.apply(rag, *srcs, *pos)


class _RagUnpackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, rag):
        tok = _c(tok)
        C = tok.shape[-1]
        dsts = [torch.empty((rag.R, L, C), dtype=tok.dtype, device=tok.device) for L in rag.lens]
        call("hdmoe_rag_unpack", dsts, tok, rag.seg, rag.lens, rag.G, rag.R, rag.Sp, C, _dt(tok))
        ctx.rag, ctx.C = rag, C
        return tuple(dsts)

    @staticmethod
    def backward(ctx, *gs):
        rag, C = ctx.rag, ctx.C
        ref = next(g for g in gs if g is not None)
        gs = [_c(g) if g is not None else torch.zeros((rag.R, L, C), dtype=ref.dtype, device=ref.device) for g, L in zip(gs, rag.lens)]
        d = torch.empty((rag.R, rag.Sp, C), dtype=ref.dtype, device=ref.device)
        call("hdmoe_rag_unpack_bwd", d, gs, rag.seg, rag.lens, rag.G, rag.R, rag.Sp, C, _dt(d))
        return d, None


def rag_unpack(tok: Tensor, rag: RagLayout):
    """Padded (R, Sp, C) -> one compact (R, S_g, C) tensor per expert (all rows: the caller selects each row's own expert later)."""
    return _RagUnpackFn.apply(tok, rag)


class _RagSelectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rag, *outs):
        outs = [_c(o) for o in outs]
        y = torch.empty_like(outs[0])
        nb = y.numel() // rag.R * y.element_size()
        call("hdmoe_rag_select", y, outs, rag.seg, rag.G, rag.R, nb)
        ctx.rag, ctx.nb = rag, nb
        return y

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        douts = [torch.empty_like(g) for _ in range(ctx.rag.G)]
        call("hdmoe_rag_select_bwd", douts, g, ctx.rag.seg, ctx.rag.G, ctx.rag.R, ctx.nb)
        return (None, *douts)


def rag_select(outs: Sequence[Tensor], rag: RagLayout) -> Tensor:
    """y[r] = outs[g(r)][r] over same-shaped per-expert tensors (R, ...)."""
    return _RagSelectFn.apply(rag, *outs)


# ---- the bank's two edges over each expert's own rows.  Rows arrive in expert-contiguous order, so expert g needs exactly the window
# [seg[g], seg[g+1]): every kernel below gets `seg[g:g+2]` (a view: the device pointer seg + g), reads the window itself and leaves all other
# rows alone -- the launches have the all-rows grid, nothing reads seg on the host, a captured graph follows each replay's routing.
# The per-expert tensors are valid inside their window only; they live inside the two nodes and never reach autograd.
VIT_BANK_ROWS = True                                    # False: patch embed / unpatch per expert over ALL rows (the path below replaces)


def vit_bank_rows_ok(x: Tensor, ws: Sequence[Tensor], E: int) -> bool:
    """Domain of the row-windowed edge kernels: bf16, contiguous square patch kernels ws[g] (E, C, p, p) that divide the image, whole
    16-byte vectors of channels (the domain of _PatchLinearFn, whose kernels the windowed entry points share)."""
    if x.dtype != torch.bfloat16 or x.ndim != 4 or not x.is_cuda:
        return False
    _, H, W, C = x.shape
    if C % 8 or E % 8:
        return False
    for w in ws:
        if w.ndim != 4 or w.shape[0] != E or w.shape[1] != C or w.shape[2] != w.shape[3] or not w.is_contiguous():
            return False
        p = int(w.shape[2])
        if H % p or W % p or (C * p * p) % 16:
            return False
    return True


def _relayout_rows(out, inp, rows, N, H, W, C, p, to_img):
    args = (out, inp, rows, N, H, W, C, p, H // p, W // p, 1, to_img, _dt(inp))
    if call("hdmoe_patch_relayout_tiled_rows", *args) == 1:
        call("hdmoe_patch_relayout_rows", *args)


def _pw_rows(x, w, y, rows, N, H, W, Cin, Ipad, Cout, flat):
    if call("hdmoe_pw_fwd_rows", x, w, y, 1.0, rows, N, H, W, Cin, Ipad, Cout, flat, _dt(x)) != 0:
        raise RuntimeError("hdmoe_pw_fwd_rows declined a shape that ops.vit_bank_rows_ok admitted")


class _VitBankEmbedFn(torch.autograd.Function):
    """Patch embedding of every expert over its own rows + pos_emb, packed: x (R,H,W,C) -> padded tokens (R,Sp,E).  Per expert the
    launches of _PatchLinearFn (relayout, GEMM, bias) with the row window, then one hdmoe_rag_pack (which reads own rows only)."""

    @staticmethod
    def forward(ctx, x, rag, *tensors):
        G = rag.G
        ws, bs, pos = tensors[:G], tensors[G:2 * G], tensors[2 * G:]
        x = _c(x)
        R, H, W, C = x.shape
        E, dt, seg = int(ws[0].shape[0]), _dt(x), rag.seg
        Epad = (E + 15) // 16 * 16
        toks, wds, ys = [], [], []
        for g in range(G):
            p = int(ws[g].shape[2])
            hp, wp, K = H // p, W // p, C * p * p
            rows = seg[g:g + 2]
            tk = torch.empty((R, hp, wp, K), dtype=x.dtype, device=x.device)
            _relayout_rows(tk, x, rows, R, H, W, C, p, 0)
            wf = torch.empty(E * K, dtype=x.dtype, device=x.device)
            wd = torch.empty(K * Epad, dtype=x.dtype, device=x.device) if ctx.needs_input_grad[0] else None
            call("hdmoe_wprep_fwd", [ws[g]], None, 1.0, [1], [1], 1, E, K, K, Epad, wf, wf.numel(), wd, 0 if wd is None else wd.numel(), 0, 0, 0, dt)
            y = torch.empty((R, hp * wp, E), dtype=x.dtype, device=x.device)
            _pw_rows(tk, wf, y, rows, R, hp, wp, K, K, E, 0)
            call("hdmoe_bias_add_rows", y, y, bs[g], rows, R, hp * wp, E, dt)
            toks.append(tk); wds.append(wd); ys.append(y)
        dst = torch.empty((R, rag.Sp, E), dtype=x.dtype, device=x.device)
        call("hdmoe_rag_pack", dst, ys, [_f32(p) for p in pos], seg, rag.lens, G, R, rag.Sp, E, dt)
        ctx.save_for_backward(*toks, *ws, *pos)
        ctx.rag, ctx.wds, ctx.dims = rag, wds, (R, H, W, C, E, Epad)
        return dst

    @staticmethod
    def backward(ctx, gt):
        rag = ctx.rag
        G, seg = rag.G, rag.seg
        saved = ctx.saved_tensors
        toks, ws, pos = saved[:G], saved[G:2 * G], saved[2 * G:]
        R, H, W, C, E, Epad = ctx.dims
        gt = _c(gt)
        dt, dev, nig = _dt(gt), gt.device, ctx.needs_input_grad
        dys = [torch.empty((R, L, E), dtype=gt.dtype, device=dev) for L in rag.lens]
        bufs, dpos = _param_grads(pos)
        call("hdmoe_rag_pack_bwd_own", dys, bufs, gt, seg, rag.lens, G, R, rag.Sp, E, dt)
        dx = None
        if nig[0]:
            dx = torch.empty((R, H, W, C), dtype=gt.dtype, device=dev)
            call("hdmoe_rag_zero_unowned", dx, seg, G, R, H * W * C * gt.element_size())
        dws, dbs = [None] * G, [None] * G
        for g in range(G):
            p = int(ws[g].shape[2])
            hp, wp, K = H // p, W // p, C * p * p
            rows = seg[g:g + 2]
            if nig[0]:
                dtok = torch.empty((R, hp, wp, K), dtype=gt.dtype, device=dev)
                _pw_rows(dys[g], ctx.wds[g], dtok, rows, R, hp, wp, E, Epad, K, 0)
                _relayout_rows(dx, dtok, rows, R, H, W, C, p, 1)
            if nig[2 + g]:
                # an expert without rows: nothing is added to the zero-initialised slab, its gradient is an exact zero
                Gs = [_zeros((1, E, K), torch.float32, dev)]
                call("hdmoe_conv_wgrad", toks[g], dys[g], Gs, rows, 1, R, hp, wp, hp, wp, K, K, E, 1, 0, [1], [1], [0], [0], dt)
                dws[g] = torch.empty_like(ws[g])
                call("hdmoe_wprep_bwd", [ws[g]], None, 1.0, Gs, [dws[g]], None, [1], [1], 1, E, K, 0)
            if nig[2 + G + g]:
                dbs[g] = torch.zeros(E, dtype=torch.float32, device=dev)
                call("hdmoe_colsum_rows", dbs[g], dys[g], rows, R, hp * wp, E, dt)
        return (dx, None, *dws, *dbs, *dpos)


def vit_bank_embed(x: Tensor, ws: Sequence[Tensor], bs: Sequence[Tensor], pos: Sequence[Tensor], rag: RagLayout) -> Tensor:
    """rag_pack([patch_embed(x, w_g, b_g) for g], pos, rag), each expert over its own rows only.  x (R,H,W,C) -> (R,Sp,E)."""
    if not vit_bank_rows_ok(x, ws, int(ws[0].shape[0])):
        raise ValueError("vit_bank_embed: outside the row-windowed kernels' domain (ops.vit_bank_rows_ok); use ops.patch_embed + ops.rag_pack")
    return _VitBankEmbedFn.apply(x, rag, *f32_params(list(ws)), *bs, *pos)


class _VitBankUnpatchFn(torch.autograd.Function):
    """rag_select([pixel_shuffle_tokens(mp_conv(part_g, w_g), ...) for part_g in rag_unpack(tok)]) with every expert over its own rows:
    the pixel shuffles write their rows of ONE image tensor (no select), the linear layers run on a window of positions."""

    @staticmethod
    def forward(ctx, tok, rag, meta, *ws):
        H, W, C, training, ps = meta
        G, seg = rag.G, rag.seg
        tok = _c(tok)
        R, Sp, E = tok.shape
        dt, dev = _dt(tok), tok.device
        parts = [torch.empty((R, L, E), dtype=tok.dtype, device=dev) for L in rag.lens]
        call("hdmoe_rag_unpack_own", parts, tok, seg, rag.lens, G, R, Sp, E, dt)
        out = torch.empty((R, H, W, C), dtype=tok.dtype, device=dev)
        call("hdmoe_rag_zero_unowned", out, seg, G, R, H * W * C * tok.element_size())
        Ipad = (E + 15) // 16 * 16
        ents, wds = [], []
        for g in range(G):
            w, L = ws[g], rag.lens[g]
            K, p = int(w.shape[0]), ps[g]
            Opad = (K + 15) // 16 * 16
            # the weight images as _MPConvFn.forward makes them for this layer (gain 1, alpha 1, normalised)
            ent = _bank.ACTIVE.lookup([w], tok.dtype, 1.0, 1.0, True) if _bank.ACTIVE is not None else None
            if ent is not None:
                wf, wd = ent.wf, ent.wd
            else:
                wf = torch.empty(K * Ipad, dtype=tok.dtype, device=dev)
                wd = torch.empty(E * Opad, dtype=tok.dtype, device=dev) if ctx.needs_input_grad[0] else None
                call("hdmoe_wprep_fwd", [w], None, 1.0, [1], [1], 1, K, E, Ipad, Opad, wf, K * Ipad, wd, E * Opad, 1, 1 if training else 0, 1, dt)
                if training:
                    _bank.note_weights_changed()
            u = torch.empty((R, L, K), dtype=tok.dtype, device=dev)
            _pw_rows(parts[g], wf, u, seg[g:g + 2], R, 1, L, E, Ipad, K, 1)
            _relayout_rows(out, u, seg[g:g + 2], R, H, W, C, p, 1)
            ents.append(ent); wds.append(wd)
        ctx.save_for_backward(*parts, *ws)
        ctx.rag, ctx.ents, ctx.wds, ctx.dims = rag, ents, wds, (R, Sp, E, H, W, C, ps)
        ctx.bank = _bank.ACTIVE
        return out

    @staticmethod
    def backward(ctx, go):
        rag = ctx.rag
        G, seg = rag.G, rag.seg
        saved = ctx.saved_tensors
        parts, ws = saved[:G], saved[G:]
        R, Sp, E, H, W, C, ps = ctx.dims
        go = _c(go)
        dt, dev, nig = _dt(go), go.device, ctx.needs_input_grad
        dparts = [torch.empty((R, L, E), dtype=go.dtype, device=dev) for L in rag.lens] if nig[0] else None
        dws = [None] * G
        for g in range(G):
            w, L, ent = ws[g], rag.lens[g], ctx.ents[g]
            K, p = int(w.shape[0]), ps[g]
            Opad = (K + 15) // 16 * 16
            rows = seg[g:g + 2]
            du = torch.empty((R, L, K), dtype=go.dtype, device=dev)
            _relayout_rows(du, go, rows, R, H, W, C, p, 0)
            if nig[0]:
                _pw_rows(du, ctx.wds[g], dparts[g], rows, R, 1, L, K, Opad, E, 1)
            if nig[3 + g]:
                if ent is not None:                            # into the weight bank's slab; the bank's finish launch makes the gradient
                    call("hdmoe_conv_wgrad", parts[g], du, list(ent.G), rows, 1, R, 1, L, 1, L, E, E, K, 1, 0, [1], [1], [0], [0], dt)
                    ctx.bank.note_backward(ent)
                else:
                    Gs = [_zeros((1, K, E), torch.float32, dev)]
                    call("hdmoe_conv_wgrad", parts[g], du, Gs, rows, 1, R, 1, L, 1, L, E, E, K, 1, 0, [1], [1], [0], [0], dt)
                    dws[g] = torch.empty_like(w)
                    call("hdmoe_wprep_bwd", [w], None, 1.0, Gs, [dws[g]], None, [1], [1], 1, K, E, 1)
        dtok = None
        if nig[0]:
            dtok = torch.empty((R, Sp, E), dtype=go.dtype, device=dev)
            call("hdmoe_rag_unpack_bwd_own", dtok, dparts, seg, rag.lens, G, R, Sp, E, dt)
        return (dtok, None, None, *dws)


def vit_bank_unpatch(tok: Tensor, ws: Sequence[Tensor], rag: RagLayout, H: int, W: int, C: int, ps: Sequence[int],
                     training: bool = False) -> Tensor:
    """Padded tokens (R,Sp,E) -> image (R,H,W,C): unpatch_proj (MP_Conv linear, weights ws[g] (C*p_g^2, E)) and the pixel shuffle of each
    row's own expert; rows of no expert are zero."""
    return _VitBankUnpatchFn.apply(tok, rag, (int(H), int(W), int(C), bool(training), tuple(int(p) for p in ps)), *f32_params(list(ws)))


class _GNRagFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rag, groups, act, eps, *params):
        x = _c(x)
        G = rag.G
        C = x.shape[-1]
        mean = torch.empty(rag.R * groups, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        y = torch.empty_like(x)
        call("hdmoe_gn_rag_fwd", y, mean, rstd, x, list(params[:G]), list(params[G:]), rag.seg, rag.lens, G, rag.R, rag.Sp, C, groups, act, eps, _dt(x))
        ctx.save_for_backward(x, mean, rstd, *params)
        ctx.meta = (rag, groups, act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, mean, rstd, *params = ctx.saved_tensors
        rag, groups, act = ctx.meta
        G = rag.G
        g = _c(g)
        dx = torch.empty_like(x)
        bufs, ret = _param_grads(params)
        call("hdmoe_gn_rag_bwd", dx, bufs[:G], bufs[G:], g, x, list(params[:G]), list(params[G:]), mean, rstd, rag.seg, rag.lens, G, rag.R, rag.Sp,
             x.shape[-1], groups, act, _dt(x))
        return (dx, None, None, None, None, *ret)


def gn_rag(x: Tensor, gammas: Sequence[Tensor], betas: Sequence[Tensor], rag: RagLayout, groups: int, act: int = 0, eps: float = 1e-5) -> Tensor:
    """nn.GroupNorm (+ activation) over each row's REAL tokens with the row's expert's affine; padding -> 0."""
    return _GNRagFn.apply(x, rag, int(groups), int(act), float(eps), *gammas, *betas)


class _LNRagFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rag, eps, *params):
        x = _c(x)
        G = rag.G
        C = x.shape[-1]
        mean = torch.empty(rag.R * rag.Sp, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        y = torch.empty_like(x)
        call("hdmoe_ln_rag_fwd", y, mean, rstd, x, list(params[:G]), list(params[G:]), rag.seg, G, rag.R, rag.Sp, C, eps, _dt(x))
        ctx.save_for_backward(x, mean, rstd, *params)
        ctx.rag = rag
        return y

    @staticmethod
    def backward(ctx, g):
        x, mean, rstd, *params = ctx.saved_tensors
        rag = ctx.rag
        G = rag.G
        g = _c(g)
        dx = torch.empty_like(x)
        bufs, ret = _param_grads(params)
        call("hdmoe_ln_rag_bwd", dx, bufs[:G], bufs[G:], g, x, list(params[:G]), mean, rstd, rag.seg, G, rag.R, rag.Sp, x.shape[-1], _dt(x))
        return (dx, None, None, *ret)


def ln_rag(x: Tensor, gammas: Sequence[Tensor], betas: Sequence[Tensor], rag: RagLayout, eps: float = 1e-5) -> Tensor:
    """nn.LayerNorm per token with the row's expert's affine."""
    return _LNRagFn.apply(x, rag, float(eps), *gammas, *betas)


class _AttnRagFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, rag, H, *biases):
        q = _c(q); k = _c(k); v = _c(v)
        R, Sp, E = q.shape
        sb = [int(b.shape[-1]) for b in biases]
        out = torch.empty_like(q)
        lse = torch.empty((R, H, Sp), dtype=torch.float32, device=q.device)
        call("hdmoe_attn_rag_fwd", out, lse, q, k, v, list(biases), rag.seg, rag.lens, sb, rag.G, R, Sp, H, E // H, _dt(q))
        ctx.save_for_backward(q, k, v, out, lse, *biases)
        ctx.meta = (rag, H, sb)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse, *biases = ctx.saved_tensors
        rag, H, sb = ctx.meta
        g = _c(g)
        R, Sp, E = q.shape
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        bufs, ret = (None, [None] * rag.G)
        if any(ctx.needs_input_grad[5:]):
            bufs, ret = _param_grads(biases)
        call("hdmoe_attn_rag_bwd", dq, dk, dv, bufs, delta, g, out, q, k, v, lse, list(biases), rag.seg, rag.lens, sb, rag.G, R, Sp, H, E // H, _dt(q))
        return (dq, dk, dv, None, None, *ret)


def attention_rag(q: Tensor, k: Tensor, v: Tensor, biases: Sequence[Tensor], rag: RagLayout, num_heads: int) -> Tensor:
    """Self-attention over each row's real tokens with the row's expert's rel_pos_bias table (H, S_g, S_g)."""
    return _AttnRagFn.apply(q, k, v, rag, int(num_heads), *biases)


def attention_rag_max_len(head_dim: int, backward: bool) -> int:
    """The longest row (tokens) attention_rag's forward / backward kernels accept at this head dim, asked of the library
    (hdmoe_attn_rag_max_len: the launchers refuse by the same expression); 0: no kernel for this head dim."""
    return int(lib().hdmoe_attn_rag_max_len(int(head_dim), 1 if backward else 0))


# =====================================================================================================
# router head + dispatch
# =====================================================================================================
class _RouterHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, noise, mask, k):
        logits = _f32(logits)
        B, E = logits.shape
        noise = None if noise is None else _f32(noise)
        mask = None if mask is None else _c(mask.to(torch.float32))
        sparse = torch.empty_like(logits)
        probs = torch.empty_like(logits)
        xout = torch.empty_like(logits)
        idx = torch.empty((B, k), dtype=torch.int32, device=logits.device)
        call("hdmoe_router_head_fwd", sparse, probs, xout, idx, logits, noise, mask, B, E, k)
        ctx.save_for_backward(sparse, probs, idx, mask)
        ctx.k = k
        ctx.mark_non_differentiable(idx)
        return sparse, probs, xout, idx

    @staticmethod
    def backward(ctx, dsparse, dprobs, dxout, _didx):
        sparse, probs, idx, mask = ctx.saved_tensors
        B, E = sparse.shape
        dl = torch.empty_like(sparse)
        call("hdmoe_router_head_bwd", dl, _c(dsparse), _c(dprobs), _c(dxout), sparse, probs, idx, mask, B, E, ctx.k)
        return dl, None, None, None


class _RouterHeadBiasFn(torch.autograd.Function):
    """The head with a selection bias (hdmoe_router_head_bias_fwd): the bias decides which experts are picked and nothing else, so it has
    no gradient and the backward is the plain head's, from the saved idx and sparse."""

    @staticmethod
    def forward(ctx, logits, noise, mask, k, sel_bias, load, target):
        logits = _f32(logits)
        B, E = logits.shape
        noise = None if noise is None else _f32(noise)
        mask = None if mask is None else _c(mask.to(torch.float32))
        sparse = torch.empty_like(logits)
        probs = torch.empty_like(logits)
        xout = torch.empty_like(logits)
        idx = torch.empty((B, k), dtype=torch.int32, device=logits.device)
        call("hdmoe_router_head_bias_fwd", sparse, probs, xout, idx, logits, noise, mask, sel_bias, load, target, B, E, k)
        ctx.save_for_backward(sparse, probs, idx, mask)
        ctx.k = k
        ctx.mark_non_differentiable(idx)
        return sparse, probs, xout, idx

    @staticmethod
    def backward(ctx, dsparse, dprobs, dxout, _didx):
        return _RouterHeadFn.backward(ctx, dsparse, dprobs, dxout, _didx) + (None, None, None)


def router_head(logits: Tensor, noise: Optional[Tensor], mask: Optional[Tensor], k: int, sel_bias: Optional[Tensor] = None,
                accum: Optional[Tuple[Tensor, Tensor]] = None):
    """masked_fill -> softmax -> top-k -> softmax(top-k) -> sparse scatter (model_components.py:158-168).
    Returns (sparse_weights, gate_probs, masked_logits, topk_idx int32).
    ``sel_bias`` (E,) fp32: the top-k runs over masked_logits + sel_bias, while the gate probabilities, the returned logits and the k gate
    weights (the softmax of the raw logits over the picked experts) stay free of it.  ``accum`` = (load, target), int64 (E,) each: the
    call adds the rows routed to every expert and 2^20 times every expert's fair share of the rows that allow it (include/hdmoe.h).
    Without a bias the call is the plain head's, whatever else is passed."""
    if sel_bias is None:
        if accum is not None:
            raise ValueError("router_head: accum needs sel_bias (the plain head does not count)")
        return _RouterHeadFn.apply(logits, noise, mask, int(k))
    E = logits.shape[-1]
    if sel_bias.dtype != torch.float32 or sel_bias.numel() != E or not sel_bias.is_contiguous() or sel_bias.device != logits.device:
        raise ValueError(f"router_head: sel_bias is a contiguous float32 tensor of {E} entries on the logits' device")
    load = target = None
    if accum is not None:
        load, target = accum
        for t in (load, target):
            if t.dtype != torch.int64 or t.numel() != E or not t.is_contiguous() or t.device != logits.device:
                raise ValueError(f"router_head: accum is a pair of contiguous int64 tensors of {E} entries on the logits' device")
    return _RouterHeadBiasFn.apply(logits, noise, mask, int(k), sel_bias, load, target)


def balance_bias_update(bias: Tensor, load: Tensor, target: Tensor, last_load: Tensor, last_target: Tensor, ok: Optional[Tensor],
                        rate: float, bias_max: float) -> None:
    """One launch (hdmoe_balance_bias_update): where ``ok`` (device int32 or None) does not read 0, bias += rate * sign(target - 2^20 load),
    re-centred and clamped to +-bias_max; always last_* = the accumulators and the accumulators = 0."""
    E = bias.numel()
    if bias.dtype != torch.float32 or not bias.is_contiguous():
        raise ValueError("balance_bias_update: bias is a contiguous float32 tensor")
    for t in (load, target, last_load, last_target):
        if t.dtype != torch.int64 or t.numel() != E or not t.is_contiguous() or t.device != bias.device:
            raise ValueError(f"balance_bias_update: the accumulators and their copies are contiguous int64 tensors of {E} entries")
    if ok is not None and (ok.dtype != torch.int32 or ok.numel() < 1 or ok.device != bias.device):
        raise ValueError("balance_bias_update: ok is an int32 tensor on the bias's device")
    call("hdmoe_balance_bias_update", bias, load, target, last_load, last_target, ok, float(rate), float(bias_max), E)


class DispatchPlan:
    """Device-side expert-contiguous permutation of the routed (sample, expert) pairs."""

    def __init__(self, sparse: Tensor, kcap: int):
        sparse = _f32(sparse.detach())
        B, E = sparse.shape
        self.B, self.E, self.kcap = B, E, int(kcap)
        self.R = B * self.kcap
        dev = sparse.device
        self.perm = torch.empty(self.R, dtype=torch.int32, device=dev)
        self.row_expert = torch.empty(self.R, dtype=torch.int32, device=dev)
        self.row_w = torch.empty(self.R, dtype=torch.float32, device=dev)
        self.inv = torch.empty(self.R, dtype=torch.int32, device=dev)
        self.seg = torch.empty(E + 1, dtype=torch.int32, device=dev)
        call("hdmoe_dispatch_plan", self.perm, self.row_expert, self.row_w, self.inv, self.seg, sparse, B, E, self.kcap)


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        x = _c(x)
        L = x.numel() // x.shape[0]
        out = torch.empty((plan.R, *x.shape[1:]), dtype=x.dtype, device=x.device)
        call("hdmoe_gather_rows", out, x, plan.perm, plan.R, L, _dt(x))
        ctx.plan = plan
        ctx.xshape = x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        g = _c(g)
        L = g.numel() // plan.R
        dx = torch.empty(ctx.xshape, dtype=g.dtype, device=g.device)
        _call_or("hdmoe_combine_rows_fwd_vec", "hdmoe_combine_rows_fwd", dx, g, plan.inv, None, plan.B, plan.kcap, L, _dt(g))
        return dx, None


def gather_rows(x: Tensor, plan: DispatchPlan) -> Tensor:
    """x[perm] : (B, ...) -> (R, ...) in expert-contiguous order (zeros in unused rows)."""
    return _GatherFn.apply(x, plan)


def gather_rows_paired(x: Tensor, plan: DispatchPlan, B: int) -> Tensor:
    """x[perm % B] : (B, ...) -> (R, ...) for a plan built over stacked copies of the B source rows (the guided evaluation's
    [conditional ; unconditional] plan over the shared stem features / time embedding); zeros in unused rows.  Inference only."""
    x = _c(x.detach())
    if x.shape[0] != B or plan.B % B != 0:
        raise ValueError(f"gather_rows_paired: {x.shape[0]} source rows, B = {B}, plan over {plan.B} rows")
    L = x.numel() // B
    out = torch.empty((plan.R, *x.shape[1:]), dtype=x.dtype, device=x.device)
    call("hdmoe_gather_rows_paired", out, x, plan.perm, plan.R, L, B, _dt(x))
    return out


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ys, sparse, plan):
        ctx.pool_ok = not sparse.is_leaf
        ys = _c(ys)
        L = ys.numel() // plan.R
        out = torch.empty((plan.B, *ys.shape[1:]), dtype=ys.dtype, device=ys.device)
        _call_or("hdmoe_combine_rows_fwd_vec", "hdmoe_combine_rows_fwd", out, ys, plan.inv, plan.row_w, plan.B, plan.kcap, L, _dt(ys))
        ctx.save_for_backward(ys)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, g):
        (ys,) = ctx.saved_tensors
        plan = ctx.plan
        g = _c(g)
        L = ys.numel() // plan.R
        dys = torch.empty_like(ys)
        dsp = _zeros((plan.B, plan.E), torch.float32, g.device, ctx.pool_ok) if ctx.needs_input_grad[1] else None
        _call_or("hdmoe_combine_rows_bwd_vec", "hdmoe_combine_rows_bwd", dys, dsp, g, ys, plan.perm, plan.row_expert, plan.row_w,
                 plan.R, plan.E, L, _dt(ys))
        return dys, dsp, None


def combine_rows(ys: Tensor, sparse: Tensor, plan: DispatchPlan) -> Tensor:
    """out[b] = sum over the rows r routed from sample b of sparse[b, e(r)] * ys[r]  (output[mask] += out*w)."""
    return _CombineFn.apply(ys, sparse, plan)


# =====================================================================================================
# small vector-path helpers (no autograd needed: inputs are data, not parameters)
# =====================================================================================================
def fourier(x: Tensor, freqs: Tensor, phases: Tensor) -> Tensor:
    """MP_Fourier.forward (model_internals.py:158-175); x must be 1-D."""
    if x.ndim != 1:
        raise RuntimeError("MP_Fourier expects a 1-D input")
    x = _f32(x.detach().to(torch.float32))
    out = torch.empty((x.shape[0], freqs.shape[0]), dtype=torch.float32, device=x.device)
    call("hdmoe_fourier", out, x, _f32(freqs), _f32(phases), x.shape[0], freqs.shape[0])
    return out


def edm_coeffs(sigma: Tensor, sigma_data: float, B: int) -> Tensor:
    """(4, B) float32: c_skip, c_out, c_in, c_noise (model_config2.py:431-438)."""
    s = _f32(sigma.detach().to(torch.float32).reshape(-1))
    coef = torch.empty((4, B), dtype=torch.float32, device=s.device)
    call("hdmoe_edm_coeffs", coef, s, s.numel(), float(sigma_data), B)
    return coef


def sigmoid_scaling(c_noise: Tensor, transition_point: float, softness: float):
    """(s_vit (B,), s_unet (B,), scaling_factors (B,2)) (model_config2.py:244-249)."""
    c = _f32(c_noise)
    B = c.shape[0]
    sv = torch.empty(B, dtype=torch.float32, device=c.device)
    su = torch.empty_like(sv)
    pair = torch.empty((B, 2), dtype=torch.float32, device=c.device)
    call("hdmoe_sigmoid_scaling", sv, su, pair, c, float(transition_point), float(softness), B)
    return sv, su, pair


# =====================================================================================================
# EDM_LOSS (row N2: the step right after the path) -- fused, sync-free
# =====================================================================================================
class _EDMLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, denoised, target, log_var, pU, pV, rU, rV, cfg):
        unet_bal, vit_bal, z_bal = cfg
        d = _f32(denoised); t = _f32(target.detach())
        B = d.shape[0]
        L = d.numel() // B
        E = pU.shape[1]
        lv = None if log_var is None else _f32(log_var).reshape(-1)
        pU, pV, rU, rV = _f32(pU), _f32(pV), _f32(rU), _f32(rV)
        out = torch.empty(5, dtype=torch.float32, device=d.device)
        aux = torch.empty(2 * E + 3, dtype=torch.float32, device=d.device)
        sse = torch.empty(B, dtype=torch.float32, device=d.device)
        call("hdmoe_edm_loss_fwd", out, aux, sse, d, t, lv, pU, pV, rU, rV, B, L, E, unet_bal, vit_bal, z_bal)
        ctx.save_for_backward(d, t, lv, rU, rV, aux, sse)
        ctx.meta = (B, L, E, cfg, None if log_var is None else log_var.shape)
        stats = out.detach()
        ctx.mark_non_differentiable(stats)
        return out[0], stats

    @staticmethod
    def backward(ctx, g, _gstats):
        d, t, lv, rU, rV, aux, sse = ctx.saved_tensors
        B, L, E, (unet_bal, vit_bal, z_bal), lv_shape = ctx.meta
        g = _f32(g.reshape(1))
        dD = torch.empty_like(d)
        dlv = None if lv is None else torch.empty_like(lv)
        dpU, dpV, drU, drV = (torch.empty_like(rU) for _ in range(4))
        call("hdmoe_edm_loss_bwd", dD, dlv, dpU, dpV, drU, drV, g, aux, sse, d, t, lv, rU, rV, B, L, E, unet_bal, vit_bal, z_bal)
        return dD, None, (None if dlv is None else dlv.reshape(lv_shape)), dpU, dpV, drU, drV, None


def edm_loss(denoised: Tensor, target: Tensor, log_var: Optional[Tensor], pU: Tensor, pV: Tensor, rU: Tensor, rV: Tensor,
             unet_bal: float, vit_bal: float, z_bal: float):
    """Returns (loss 0-dim with grad, stats (5,) detached = [loss, denoising, balance, z_loss, pure_loss])."""
    return _EDMLossFn.apply(denoised, target, log_var, pU, pV, rU, rV, (float(unet_bal), float(vit_bal), float(z_bal)))
