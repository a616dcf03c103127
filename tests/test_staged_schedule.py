"""Host-only checks of the staged step's stage table (hdmoe_hip/graph.py STEP) and of what is derived from it: the legal stage
sequences, the capture order of the backward sections and the replay schedule.  No stream is created; the schedule is run through a
happens-before simulator and compared with traces recorded from the hand-written replay this table replaced (its StagedStep.__call__
driven on fake streams, graphs and hooks)."""
import pytest

from hdmoe_hip.graph import STEP, KIND, order, sections, schedule
from hdmoe_hip.dp import GradBuckets

# ("wait", a, b): stream a waits for stream b; ("run" | "done", stage, stream).  One replay each; every replay is the same list.
PARENT = {
    "A": (   # 36 records
        ('wait', 'main', 'cur'), ('run', 'pre', 'main'), ('wait', 'u', 'main'), ('wait', 'v', 'main'), ('run', 'ur', 'u'), ('run', 'vit', 'v'),
        ('wait', 'u', 'main'), ('wait', 'u', 'u'), ('run', 'unet', 'u'), ('wait', 'main', 'u'), ('wait', 'main', 'v'), ('run', 'post', 'main'),
        ('wait', 'u', 'main'), ('wait', 'v', 'main'), ('run', 'ucomb_bwd', 'u'), ('run', 'vcomb_bwd', 'v'), ('wait', 'r', 'u'),
        ('run', 'unet_bwd', 'u'), ('run', 'ur_bwd', 'r'), ('wait', 'main', 'v'), ('run', 'vr_bwd', 'main'), ('run', 'vit_bwd', 'v'),
        ('wait', 'v', 'main'), ('done', 'unet_bwd', 'u'), ('run', 'unet_bwd2', 'u'), ('done', 'unet_bwd2', 'u'), ('run', 'unet_bwd1', 'u'),
        ('done', 'unet_bwd1', 'u'), ('run', 'unet_bwd0', 'u'), ('done', 'vit_bwd', 'v'), ('wait', 'u', 'r'), ('done', 'unet_bwd0', 'u'),
        ('wait', 'main', 'u'), ('wait', 'main', 'v'), ('run', 'pre_bwd', 'main'), ('wait', 'cur', 'main'),
    ),
    "B": (   # 30 records
        ('wait', 'main', 'cur'), ('run', 'pre', 'main'), ('wait', 'u', 'main'), ('wait', 'v', 'main'), ('run', 'ur', 'u'), ('run', 'vit', 'v'),
        ('wait', 'u', 'main'), ('wait', 'u', 'u'), ('run', 'unet', 'u'), ('wait', 'main', 'u'), ('wait', 'main', 'v'), ('run', 'post', 'main'),
        ('wait', 'u', 'main'), ('wait', 'v', 'main'), ('run', 'ucomb_bwd', 'u'), ('run', 'vcomb_bwd', 'v'), ('wait', 'r', 'u'),
        ('run', 'unet_bwd', 'u'), ('run', 'ur_bwd', 'r'), ('wait', 'main', 'v'), ('run', 'vr_bwd', 'main'), ('run', 'vit_bwd', 'v'),
        ('wait', 'v', 'main'), ('done', 'vit_bwd', 'v'), ('wait', 'u', 'r'), ('done', 'unet_bwd', 'u'), ('wait', 'main', 'u'), ('wait', 'main', 'v'),
        ('run', 'pre_bwd', 'main'), ('wait', 'cur', 'main'),
    ),
    "C": (   # 19 records
        ('wait', 'main', 'cur'), ('run', 'pre', 'main'), ('wait', 'u', 'main'), ('wait', 'v', 'main'), ('run', 'unet', 'u'), ('run', 'vit', 'v'),
        ('wait', 'main', 'u'), ('wait', 'main', 'v'), ('run', 'post', 'main'), ('wait', 'u', 'main'), ('wait', 'v', 'main'),
        ('run', 'unet_bwd', 'u'), ('run', 'vit_bwd', 'v'), ('done', 'vit_bwd', 'v'), ('done', 'unet_bwd', 'u'), ('wait', 'main', 'u'),
        ('wait', 'main', 'v'), ('run', 'pre_bwd', 'main'), ('wait', 'cur', 'main'),
    ),
}
SUB = ["unet_bwd2", "unet_bwd1", "unet_bwd0"]
FWD_R, FWD = ["pre", "ur", "unet", "vit", "post"], ["pre", "unet", "vit", "post"]
BWD_R = ["ucomb_bwd", "unet_bwd", "ur_bwd", "vcomb_bwd", "vit_bwd", "vr_bwd", "pre_bwd"]
CAPTURE = {"A": FWD_R + BWD_R[:2] + SUB + BWD_R[2:], "B": FWD_R + BWD_R, "C": FWD + ["unet_bwd", "vit_bwd", "pre_bwd"]}
PRODUCER = {"ucomb_bwd": "ucomb", "unet_bwd": "unet", "unet_bwd2": "unet_c2", "unet_bwd1": "unet_c1", "unet_bwd0": "unet_c0", "ur_bwd": "ur",
            "vcomb_bwd": "vcomb", "vit_bwd": "vit", "vr_bwd": "vr", "pre_bwd": "pre"}
# the local cuts (Stager.cut_local / the keywords of the `post` cut) the model makes in each shape
LOCAL_CUTS = {"A": {"ucomb", "vcomb", "vr", "unet_c2", "unet_c1", "unet_c0"}, "B": {"ucomb", "vcomb", "vr"}, "C": set()}


def simulate(ops, replays=2):
    """[(replay, kind, stage, stream, frozenset of the (replay, kind, stage) ordered before it)] of ``replays`` runs of ``ops``."""
    before = {}
    out = []
    for n in range(replays):
        for kind, a, b in ops:
            if kind == "wait":
                before[a] = before.get(a, frozenset()) | before.get(b, frozenset())
            else:
                out.append((n, kind, a, b, before.get(b, frozenset())))
                before[b] = before.get(b, frozenset()) | {(n, kind, a)}
    return out


@pytest.mark.parametrize("shape", "ABC")
def test_schedule_orders_what_the_parent_replay_ordered(shape):
    got, want = simulate(schedule(shape)), simulate(PARENT[shape])
    assert [g[:4] for g in got] == [w[:4] for w in want]            # issue order of launches and hooks, and their streams
    for g, w in zip(got, want):
        assert g[4] == w[4], (g[:4], sorted(g[4] - w[4]), sorted(w[4] - g[4]))   # (extra serialisation, missing edges)
    assert len(schedule(shape)) <= len(PARENT[shape])
    assert not any(k == "wait" and a == b for k, a, b in schedule(shape))


@pytest.mark.parametrize("shape", "ABC")
def test_stage_sequences_and_capture_order(shape):
    want = CAPTURE[shape]
    assert order(shape) == want
    fwd = want[:want.index("post") + 1]
    bwd = want[len(fwd):]
    assert sections(fwd, LOCAL_CUTS[shape]) == [(s, PRODUCER[s]) for s in bwd]
    assert all(KIND[s] in ("main", "u", "v", "r") for s in want)
    assert {r.name: r.producer for r in STEP if r.producer} == PRODUCER


def test_partial_unet_split_is_no_legal_sequence():
    from hdmoe_hip.graph import StagedStep
    assert StagedStep.ORDER == CAPTURE["C"]
    assert StagedStep.ORDER_R == ["pre", "ur", "unet", "vit", "post", "ucomb_bwd", "unet_bwd", "ur_bwd", "vit_bwd", "pre_bwd"]
    legal = [order(s) for s in "ABC"]
    for keep in (["unet_bwd2"], ["unet_bwd2", "unet_bwd1"], ["unet_bwd1", "unet_bwd0"], ["unet_bwd0"]):
        seq = [s for s in CAPTURE["A"] if s not in SUB or s in keep]
        assert seq not in legal
        cuts = LOCAL_CUTS["B"] | {PRODUCER[s] for s in keep}       # ... and it is what such a forward would capture
        assert FWD_R + [s for s, _ in sections(FWD_R, cuts)] == seq


@pytest.mark.parametrize("shape", "ABC")
def test_data_dependencies_are_ordered(shape):
    """From the model's cuts (models/_assembly.py, model_components.py), not from the table: who reads whose tensors."""
    deps = [("ur", "pre"), ("vit", "pre"), ("unet", "pre"), ("unet", "ur"), ("post", "unet"), ("post", "vit"), ("post", "ur")]
    deps += [(s, "post") for s in PRODUCER]
    deps += [(s, "ucomb_bwd") for s in ["unet_bwd", "ur_bwd"] + SUB]
    deps += [("unet_bwd2", "unet_bwd"), ("unet_bwd1", "unet_bwd2"), ("unet_bwd0", "unet_bwd1")]
    deps += [("vit_bwd", "vcomb_bwd"), ("vr_bwd", "vcomb_bwd")]
    deps += [("pre_bwd", s) for s in PRODUCER if s != "pre_bwd"]
    have = set(CAPTURE[shape])
    sim = {(n, kind, s): pred for n, kind, s, _, pred in simulate(schedule(shape))}
    checked = set()
    for n in (0, 1):
        for later, earlier in deps:
            if later in have and earlier in have:
                assert (n, "run", earlier) in sim[(n, "run", later)], (n, later, earlier)
                checked.add(later)
    assert checked == have - {"pre"}                                # every stage of the shape has a dependency that was looked at
    assert (0, "run", "pre_bwd") in sim[(1, "run", "pre")]          # the next replay's stem waits for this one's last section
    assert all((0, "run", "pre_bwd") in pred for (n, _, _), pred in sim.items() if n == 1)


class _Staged:
    def __init__(self, unet_sub):
        self.unet_sub = unet_sub


class _Log:
    def __init__(self):
        self.tags = []

    def launch_tag(self, tag):
        self.tags.append(tag)


def _fire(shape, unet_sub):
    """Tags in the order the schedule of ``shape`` fires the hooks of GradBuckets.staged_hooks, and each hook's predecessors."""
    log = _Log()
    hooks = GradBuckets.staged_hooks(log, _Staged(unet_sub))
    pred = {}
    for n, kind, stage, _, before in simulate(schedule(shape), replays=1):
        if kind == "done" and stage in hooks:
            at = len(log.tags)
            hooks[stage]()
            for tag in log.tags[at:]:
                pred[tag] = before
    return log.tags, pred, hooks


def test_hooks_fire_in_bucket_order_behind_the_router_sections():
    tags, pred, hooks = _fire("A", SUB)
    assert tuple(tags) == GradBuckets.TAGS[:-1] and GradBuckets.TAGS[-1] == "rest"
    assert set(hooks) == {s for _, kind, s, _, _ in simulate(schedule("A"), 1) if kind == "done"}      # every hook has its point in the replay
    assert (0, "run", "vr_bwd") in pred["vit"] and (0, "run", "vit_bwd") in pred["vit"]
    assert (0, "run", "ur_bwd") in pred["unet_s0"] and (0, "run", "unet_bwd0") in pred["unet_s0"]
    for tag, sec in (("unet_s3", "unet_bwd"), ("unet_s2", "unet_bwd2"), ("unet_s1", "unet_bwd1")):
        assert (0, "run", sec) in pred[tag]
    for shape in "BC":                                              # one U-Net section: all of its buckets behind it and behind the router's
        tags, pred, _ = _fire(shape, [])
        assert tags == ["vit", "unet_s3", "unet_s2", "unet_s1", "unet_s0"]
        assert all((0, "run", "unet_bwd") in pred[t] for t in tags[1:]) and (0, "run", "vit_bwd") in pred["vit"]
        if shape == "B":
            assert (0, "run", "ur_bwd") in pred["unet_s0"] and (0, "run", "vr_bwd") in pred["vit"]


def test_staged_hooks_refuse_a_partial_unet_split():
    for sub in (["unet_bwd2"], ["unet_bwd2", "unet_bwd1"]):
        with pytest.raises(RuntimeError):
            GradBuckets.staged_hooks(_Log(), _Staged(sub))
