"""hipGraph capture of a whole training step (forward + loss + backward + weight-gradient finish).

The step issues ~2.4k kernel launches from Python; once the kernels are fast the host becomes the bottleneck.  Every op of the
path is sync-free and allocation goes through torch's caching allocator, so the step can be captured once with
``torch.cuda.graph`` and replayed; randomness stays fresh across replays through the device-side step counter
(`ops.advance_seed`), and parameters / gradient buckets keep their addresses.
"""
from __future__ import annotations

import collections
import contextlib
import os
import time

import torch

from . import bank, ops


def _capture_mode() -> str:
    """Error mode of the stream captures.  With a process group alive (RCCL's watchdog thread polls events from its own thread)
    a 'global' capture would turn that polling into a capture error; 'thread_local' restricts the check to the capturing thread.
    The step allocates nothing new after its warm-up runs, so the laxer mode hides nothing."""
    import torch.distributed as dist
    return "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"


@contextlib.contextmanager
def no_gc():
    """Python's cyclic collector must not run inside a stream capture: collecting a dead graph, stream or event of an EARLIER capture (a
    test's StagedStep, a sampler's stage graphs -- all cycles) calls hipGraphDestroy / hipEventDestroy from the capturing thread, the
    runtime refuses that inside a global-mode capture and the destructor's exception ends the process ("Fatal Python error: Aborted ...
    Garbage-collecting" in the middle of a capture, once in a few hundred runs).  Collect before, keep the collector off until the end."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class GraphedStep:
    def __init__(self, step_fn, device, warmup: int = 3):
        """``step_fn()`` must be re-runnable with static inputs and write its results into persistent tensors."""
        self.device = torch.device(device)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):                      # registers the weight bank, sizes the allocator pool
                ops.advance_seed(self.device)
                step_fn()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        self.graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(self.graph, capture_error_mode=_capture_mode()):
            ops.advance_seed(self.device)
            self.out = step_fn()
            bank.join_forked_streams()                  # every forked side stream is back on the capture stream

    def __call__(self):
        self.graph.replay()
        return self.out


# =====================================================================================================================================
# Staged capture: one hipGraph per independent section of the step, the two expert branches replayed on separate streams.
#
# The two expert branches of HDMOEM (router + U-Net bank / router + ViT bank) are independent between the stem and the fusion, and
# most of their kernels are far too small to fill 256 CUs.  The step is cut at those two points -- in the forward AND in the
# backward -- into seven graphs:
#
#     pre (stem, scaling, time embedding)  ->  unet | vit  ->  post (fusion, head, loss, and their backward)
#                                          ->  unet_bwd | vit_bwd  ->  pre_bwd (stem backward, weight-bank finish)
#
# and the host launches `unet` / `vit` (and the two backward graphs) on two streams, ordered by events.  Autograd is cut with
# detached leaves at the stage boundaries; each backward section is an explicit torch.autograd.backward call over the boundary
# tensors of its stage, so every section is captured on the stream its forward ran on.
#
# Measured on MI355X (BASELINE configs[1], same box, un-profiled): single stream 21.4 ms, ONE graph with the ViT bank forked onto a
# side stream 19.4 ms, staged 19.2 ms.  So a fork inside one graph already overlaps; what the staged form adds is (a) ~1 % of step
# time, (b) HIP events BETWEEN the graphs, i.e. per-stage GPU times without a profiler (`stage_times()`, bench.py "stage_ms"), and
# (c) host-visible points between the backward sections where finished gradient buckets can be handed to RCCL while the rest of the
# backward still runs.  A warning that cost hours: a rocprofv3 --kernel-trace timeline of the replay shows the branches strictly one
# after the other -- the tracer adds ~17-20 us of host time per dispatch, the replay becomes host-bound and the queues drain in
# issue order.  Branch overlap has to be read from events (stage_ms), not from the trace.
# =====================================================================================================================================
# The step, one row per graph launch ("run") or hook point ("done": StagedStep.after[name] runs there, on that section's stream -- e.g.
# dp.GradBuckets.launch_tag hands the section's gradient bucket to RCCL), in the order the host issues them in a replay.  Everything else
# is derived from this table: the stream of each stage (KIND), the legal stage sequences of a capture (order), the backward sections
# and the order they are captured in (sections) and the replay itself (schedule).
#   shapes    which forms of the step contain the row.  A: SPLIT_ROUTER with the U-Net bank's backward in four sections (15 graphs; the
#             trainer and bench.py); B: SPLIT_ROUTER with a one-level U-Net (12 graphs); C: the seven-graph form (tests set
#             Stager.SPLIT_ROUTER = False).  `unet` and the hook of `unet_bwd` are issued at a different point in A / B / C: two rows.
#   waits     (a, b[, shapes]): stream a waits for everything issued to stream b so far, right before the row; "cur" is the caller's
#             stream.  A replay ends with cur waiting for main.
#   producer  backward sections: the key of the cuts (Stager.cut / cut_local) whose leaves the section differentiates.
#   cap       position in the capture: the order the stages are captured in (which decides the allocation inside the per-stream graph
#             pools) differs from the replay's issue order.
Row = collections.namedtuple("Row", "op name stream shapes waits producer cap", defaults=((), None, None))
STEP = (
    Row("run", "pre", "main", "ABC", (("main", "cur"),), cap=0),
    Row("run", "unet", "u", "C", (("u", "main"),), cap=2),
    # The router FORWARD of the U-Net branch is on the critical path (the bank cannot start before the routing weights exist): it runs
    # on the bank's own stream; only its backward, which has slack, uses the third stream.
    Row("run", "ur", "u", "AB", (("u", "main"),), cap=1),
    Row("run", "vit", "v", "ABC", (("v", "main"),), cap=3),
    Row("run", "unet", "u", "AB", (), cap=2),                      # (behind `ur` on its stream)
    Row("run", "post", "main", "ABC", (("main", "u"), ("main", "v")), cap=4),
    Row("run", "ucomb_bwd", "u", "AB", (("u", "main"),), "ucomb", 5),
    Row("run", "vcomb_bwd", "v", "AB", (("v", "main"),), "vcomb", 11),
    # (the router's backward waits for the combine backward only: its wait is issued BEFORE the bank's backward goes to stream u)
    Row("run", "unet_bwd", "u", "ABC", (("u", "main", "C"), ("r", "u", "AB")), "unet", 6),
    Row("run", "ur_bwd", "r", "AB", (), "ur", 10),
    # SPLIT_VROUTER, the ViT router's backward as its own section (round 4, always on): with the U-Net bank's backward down to ~6 ms the ViT section became the LAST one to finish (stage_ms: vit_bwd
    # 6.2 -> 12.8 ms, unet_bwd0 ends at 12.4): its stream runs the ViT bank's backward (~170 small launches) and then the ViT router's trunk
    # backward (the heavy part) one after the other.  The router's backward needs only the gradient of the routing weights, which the
    # combine backward -- the section's first kernel -- produces: same cut as for the U-Net router (`vcomb_bwd` on the ViT stream, then
    # `vr_bwd` beside `vit_bwd`).  The forward stays one graph.  The stream of `vr_bwd`, same box, ms/step, with the stream
    # priorities of the time: no split 13.39; "r" (behind the U-Net router's backward) 13.13; "main" (idle between `post` and `pre_bwd`) 13.32;
    # "r2" (a fifth stream of our own) 17.9 -- see the note on hardware queues in StagedStep.  Without priorities (the default now, see StagedStep):
    # "main" 13.02, "r" 13.62.
    Row("run", "vr_bwd", "main", "AB", (("main", "v"),), "vr", 13),   # (behind the combine backward)
    Row("run", "vit_bwd", "v", "ABC", (("v", "main", "C"),), "vit", 12),
    # SPLIT_UNET_BWD (round 4, always on): the U-Net bank's backward as up to FOUR sections on its stream -- decoder at full resolution (+ output conv),
    # decoder below, encoder below, encoder at full resolution (+ embeddings) -- cut with detached leaves inside the forward graph
    # (models/model_components.py unet_expert_bank_forward).  Each section finishes its own weight gradients (bank.finish_stage), so its
    # gradient bucket can go to RCCL while the later sections still run (hdmoe_hip/dp.py); single-process jobs just replay four graphs.
    # The bank's sections one after the other on its stream; behind each the hook that hands its gradient bucket on
    # (buckets are ordered by completion: decoder sections first, then the ViT branch, then what ends with the backward).
    Row("done", "unet_bwd", "u", "A"),
    Row("run", "unet_bwd2", "u", "A", (), "unet_c2", 7),
    Row("done", "unet_bwd2", "u", "A"),
    Row("run", "unet_bwd1", "u", "A", (), "unet_c1", 8),
    Row("done", "unet_bwd1", "u", "A"),
    Row("run", "unet_bwd0", "u", "A", (), "unet_c0", 9),
    Row("done", "vit_bwd", "v", "ABC", (("v", "main", "AB"),)),    # the "vit" gradient bucket holds the ViT router's parameters too: behind `vr_bwd`
    Row("done", "unet_bwd0", "u", "A", (("u", "r"),)),             # the last U-Net bucket holds the router's parameters too: behind `ur_bwd`
    Row("done", "unet_bwd", "u", "BC", (("u", "r", "B"),)),        # the "unet" gradient bucket holds the router's parameters too
    Row("run", "pre_bwd", "main", "ABC", (("main", "u"), ("main", "v")), "pre", 14),
)
KIND = {r.name: r.stream for r in STEP if r.op == "run"}


def order(shape: str) -> list:
    """The stage sequence a capture of ``shape`` must produce."""
    return [r.name for r in sorted((r for r in STEP if r.op == "run" and shape in r.shapes), key=lambda r: r.cap)]


def sections(ran, cuts_present) -> list:
    """[(backward section, producer key)] behind `post`, in capture order, for a forward that ran the stages ``ran`` and made the local
    cuts ``cuts_present``: a section exists when its producer does."""
    rows = sorted((r for r in STEP if r.producer is not None), key=lambda r: r.cap)
    return [(r.name, r.producer) for r in rows if r.producer in ran or r.producer in cuts_present]


def schedule(shape: str) -> list:
    """The replay of ``shape`` as a flat list of ("wait", a, b) -- stream a waits for stream b -- / ("run", stage, stream) /
    ("done", stage, stream); streams by name."""
    ops = []
    for r in STEP:
        if shape in r.shapes:
            ops += [("wait", a, b) for a, b, *only in r.waits if not only or shape in only[0]]
            ops.append((r.op, r.name, r.stream))
    return ops + [("wait", "cur", "main")]


class Stager:
    """Stage bookkeeping shared by the eager warm-up runs and the capture run of a StagedStep.  Model code talks to it through
    ``graph.current()``: ``cut(stage, **tensors_by_producer_stage)`` at a boundary, ``backward(loss)`` instead of loss.backward()."""

    # SPLIT_ROUTER: the U-Net branch is the longer one, and its router's backward (2.2 ms of kernels) needs nothing from the bank's
    # backward but the gradient of the routing weights, which the bank's FIRST backward kernel (the combine) produces.  The router
    # therefore gets its own stream and graphs (`ur`, `ur_bwd`), and the combine backward its own small graph (`ucomb_bwd`) so that
    # `ur_bwd` can start right after it, beside the bank backward.  (Tests set it False to compare against the seven-graph form.)
    SPLIT_ROUTER = True

    def __init__(self, device, streams, pools):
        self.device, self.streams, self.pools = device, streams, pools
        self.capture = False
        self.graphs = {}
        self.stage = None
        self._ctx = None
        self.cuts = collections.defaultdict(list)                # producer segment -> [(tensor, detached leaf)]
        self.order = []

    # -- stage switching ------------------------------------------------------------------------------------------------------
    def begin(self, name: str):
        assert self.stage is None
        st = self.streams[KIND[name]]
        if self.capture:
            g = torch.cuda.CUDAGraph()
            self.graphs[name] = g
            self._ctx = torch.cuda.graph(g, pool=self.pools[KIND[name]], stream=st, capture_error_mode=_capture_mode())
        else:
            for other in self.streams.values():                  # warm-up: plain streams, fully ordered
                st.wait_stream(other)
            self._ctx = torch.cuda.stream(st)
        self._ctx.__enter__()
        self.stage = name
        self.order.append(name)

    def end(self):
        if self.stage is not None:
            self._ctx.__exit__(None, None, None)
            self.stage, self._ctx = None, None

    def cut(self, stage: str, **by_producer):
        """End the current stage, begin ``stage``; tensors that need a gradient are replaced by detached leaves (their gradients
        are fed to the producer stage's backward section later).  Returns the tensors in keyword order, flattened."""
        self.end()
        self.begin(stage)
        return self.cut_local(**by_producer)

    def cut_local(self, **by_producer):
        """Detached leaves without a stage switch: a boundary between two backward sections inside one forward graph."""
        out = []
        for producer, tensors in by_producer.items():
            for t in tensors:
                if torch.is_tensor(t) and t.requires_grad and not (t.is_leaf and producer.startswith("unet_c")):
                    # (inside the U-Net bank a tensor that already IS a boundary leaf stays one: no chains of leaves)
                    d = t.detach().requires_grad_(True)
                    self.cuts[producer].append((t, d))
                    out.append(d)
                else:
                    out.append(t)
        return out

    def _section(self, stage: str, producer: str):
        self.end()
        self.begin(stage)
        bank.STAGE = stage
        pairs = [(t, d.grad) for t, d in self.cuts[producer] if d.grad is not None]
        if pairs:
            torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
        if stage != "pre_bwd":
            bank.finish_stage(stage)                              # this section's weight gradients are final when its graph ends

    def backward(self, loss):
        if "post" not in self.order:
            raise RuntimeError("staged step: the model did not reach its stage boundaries (not the banked HDMOEM path)")
        bank.DEFER_FINISH = True
        try:
            bank.STAGE = "post"
            loss.backward()                                       # fusion + head + loss section; stops at the detached leaves
            for stage, producer in sections(self.order, {k for k, v in self.cuts.items() if v}):
                self._section(stage, producer)
        finally:
            bank.DEFER_FINISH = False
            bank.STAGE = None
        bank.finish_pending()                                     # the remaining weight gradients (stem, fusion, head): last section


_ACTIVE = None


def current():
    """The active Stager (inside a StagedStep run) or None."""
    return _ACTIVE


def backward(loss):
    """loss.backward(), or the staged backward sections when a StagedStep is running."""
    if _ACTIVE is not None:
        _ACTIVE.backward(loss)
    else:
        loss.backward()


class StagedStep:
    """Drop-in for GraphedStep when ``step_fn`` runs the banked HDMOEM path and calls ``graph.backward(loss)``.

    Two keyword arguments exist for timing / race experiments only (tools/replay_race.py): ``priorities=True`` gives the U-Net and main
    streams the higher priority (see the note in __init__), ``skip`` names sections that every replay drops -- the step's results are
    then WRONG."""

    ORDER = order("C")                                                         # the seven-graph form
    ORDER_R = [n for n in order("B") if n not in ("vcomb_bwd", "vr_bwd")]      # SPLIT_ROUTER, without the sections of SPLIT_VROUTER / SPLIT_UNET_BWD

    def __init__(self, step_fn, device, warmup: int = 3, *, priorities: bool = False, skip=()):
        self.device = torch.device(device)
        self.skip = tuple(skip)
        # the U-Net branch is the longer one (the ViT branch has ~2.5 ms of slack in the backward): its stream gets the higher priority
        # ... but only in a single-process job.  Measured with a one-rank RCCL group (bench.py HDMOE_BENCH_FORCE_DIST=1): as soon as the
        # process owns one more stream (RCCL's) next to prioritised ones, whole stages run 1.5-2x longer (17.3 -> 22.5 ms/step; a fifth
        # stream of our own did the same); with equal priorities the extra stream costs ~0.2 ms (17.2 vs 17.0 ms/step including the
        # all-reduces).  How ROCclr maps streams onto its hardware queues
        # (GPU_MAX_HW_QUEUES, default 4 per priority level) decides whether two of our streams end up sharing a queue and whole
        # stages serialise: measured under the one-rank RCCL group 4 queues 17.2, 8 queues 17.4, 6 queues 20.4 ms/step; without a group
        # and without priorities 4 queues 18.0, 8 queues 17.6; a ONE-graph replay with an internal fork (the sampler) is 20 % slower
        # with 8 queues than with 4.  The default (4) is the best setting for every configuration the code itself selects.
        # ROUND 4: stream priorities are OFF unless `priorities=True` (tools/replay_race.py).  With prioritised streams, replays launched
        # back to back (the host a replay ahead of the device -- what a training loop and bench.py do) showed a transient: in 2-6 % of the replays the router logits of the LOW-priority branch
        # came out with a bf16-sized error (5e-3 .. 3e-2 against 8e-5), gone in the next replay (tools/replay_race.py: 51 outliers in 900 bursts of
        # three replays; 0 in 1800 bursts without priorities, 0 with a synchronize between the replays; it survives dropping every backward section
        # from the replay, so it sits between `pre` / the forward branches of neighbouring replays).  The event dependencies are the same either
        # way; which wait the prioritised queues do not honour was not isolated.  Without priorities the schedule needs `vr_bwd` on the `main`
        # stream to keep the step time (12.98 prioritised, 13.02 equal priorities + vr_bwd on main, 13.62 equal priorities + vr_bwd behind ur_bwd).
        prio = {"main": -1, "u": -1, "v": 0, "r": 0} if priorities else {"main": 0, "u": 0, "v": 0, "r": 0}
        names = ("main", "u", "v", "r")
        self.streams = {k: torch.cuda.Stream(device=self.device, priority=prio[k]) for k in names}
        self.pools = {k: torch.cuda.graph_pool_handle() for k in names}
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams.values():
            s.wait_stream(cur)
        for _ in range(warmup):
            self._run(step_fn, capture=False)
        for s in self.streams.values():
            cur.wait_stream(s)
        torch.cuda.synchronize(self.device)
        with no_gc():
            st = self._run(step_fn, capture=True)
        shape = next((k for k in "ABC" if st.order == order(k)), None)
        if shape is None:
            raise RuntimeError(f"staged step: unexpected stage sequence {st.order}")
        self.split_router = shape != "C"
        self.unet_sub = ["unet_bwd2", "unet_bwd1", "unet_bwd0"] if shape == "A" else []   # further sections of the U-Net bank's backward
        self._ops = schedule(shape)
        self.graphs = st.graphs
        self._keep = st                                           # boundary tensors live in the graphs' pools
        self.after = {}                                           # {section with a "done" row in STEP: callable}: run on that section's stream behind its launch
        self.host_us = {} if os.environ.get("HDMOE_HOST_TIMES") == "1" else None

    def _run(self, step_fn, capture: bool):
        global _ACTIVE
        st = Stager(self.device, self.streams, self.pools)
        st.capture = capture
        _ACTIVE = st
        try:
            st.begin("pre")
            ops.advance_seed(self.device)
            self.out = step_fn()
        finally:
            try:
                st.end()
            finally:
                _ACTIVE = None
        return st

    def __call__(self):
        g = self.graphs
        ev = self._events = {} if self.timing else None

        skip = self.skip

        def run(name, stream):
            if name in skip:
                if ev is not None:
                    ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[name][0].record(stream); ev[name][1].record(stream)
                return
            with torch.cuda.stream(stream):
                if ev is not None:
                    ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[name][0].record(stream)
                if self.host_us is None:
                    g[name].replay()
                else:                                             # development: host time of the graph launch itself (HDMOE_HOST_TIMES=1)
                    t0 = time.perf_counter()
                    g[name].replay()
                    self.host_us[name] = self.host_us.get(name, 0.0) + (time.perf_counter() - t0) * 1e6
                    self.host_us["_calls_" + name] = self.host_us.get("_calls_" + name, 0) + 1
                if ev is not None:
                    ev[name][1].record(stream)

        def done(name, stream):                                   # e.g. hand the section's gradient bucket to RCCL (dp.GradBuckets.launch_tag)
            fn = self.after.get(name)
            if fn is not None:
                with torch.cuda.stream(stream):
                    fn()

        S = dict(self.streams, cur=torch.cuda.current_stream(self.device))
        for op, name, stream in self._ops:
            if op == "wait":
                S[name].wait_stream(S[stream])
            elif op == "run":
                run(name, S[stream])
            else:
                done(name, S[stream])
        return self.out

    timing = False

    def stage_times(self):
        """(after a call with ``timing = True`` and a synchronize) {stage: (start ms, end ms)} relative to the start of `pre`."""
        t0 = self._events["pre"][0]
        return {k: (round(t0.elapsed_time(a), 3), round(t0.elapsed_time(b), 3)) for k, (a, b) in self._events.items()}
