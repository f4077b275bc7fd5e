"""Sequences of frames around repeat TriangleBuffer draws against the CPU
oracle, bit for bit: after every recorded frame the f64 framebuffer, the u32
depth and the u8 image or frame output (u8 image / YUV420P planes) of every
context, and the fragment counts while counting is on.

A sequence is plain data of tests/frame_seq.py's vocabulary, run by its one
interpreter on the library and on the oracle: the context lives for the whole
sequence, so a frame's pixels depend on what earlier frames left in the warm
schedule, the kept pair list and the visible list -- frames that accumulate
without clears, several buffers and other batches in one frame, RGBA contexts,
shard changes, knobs flipped between repeats, resize and back, a buffer
destroyed and made again, two contexts, frames nobody reads, transforms at the
loose binning's 2 px boundary.  tests/test_frame_seq.py checks, on exactly the
examples drawn here, that the generated sequences hold all of that.

Two property tests draw the sequences (hypothesis, derandomized).  Reached
records which shortcut every buffer draw took and is asserted at each test's
end, so the fuzz cannot go vacuous.  FIXED names the hand-offs one by one, in
the same data, so that a failing fuzz sequence (printed with the frame and the
counters) can be added as one more entry.

No fault injection here (tests/test_warm_gpu.py, test_list_reuse_gpu.py and
test_visible_list_gpu.py inject faults): every sequence must end with no warm
failure and no latched error.

Running time, measured with --durations on one MI355X (call phase, several runs):
    test_random_sequences_match_oracle          1.3-1.5 s alone, 1.08 s within the whole suite (64 sequences, 841 frames)
    test_random_large_sequences_match_oracle    1.01 s, 1.05 s, 1.08 s (3 sequences of 350 000 triangles, 34 frames)
    test_fixed_sequence                         0.02 s each (0.13 s for the first one of a process)
The example counts (frame_seq.SMALL_EXAMPLES = 64, LARGE_EXAMPLES = 3) are above the floors of 40 small sequences
with 400 frames and 2 large ones, and keep each test below the largest fuzz test before it (1.7 s).
"""
import collections

import hypothesis  # noqa: F401  (a missing package fails the module: these tests never skip)
import pytest

import frame_seq as S

pytestmark = pytest.mark.gpu

W, H = 200, 140            # 4 x 5 tiles, partial right and bottom tiles
BINS = ("cold", "warm", "loose")


class Reached:
    """Which shortcut the buffer draws of one property test took (the "how"
    of frame_seq.run's draws), and under what."""

    def __init__(self):
        self.hit = collections.Counter()
        self.sequences = self.frames = 0

    def note(self, seq, got):
        _, _, alpha, knobs, specs, frames = seq
        self.sequences += 1
        self.frames += len(frames)
        by_frame = collections.defaultdict(list)
        for d in got["draws"]:
            by_frame[d["frame"]].append(d)
        cur, split = 0, {0: knobs["split"], 1: knobs["split"]}
        history = collections.defaultdict(list)          # (context, buffer) -> how, draw by draw
        pruned_in = {}                                   # (context, buffer) -> depth mode of its visible list
        for k, (ops, read) in enumerate(frames):
            for op in ops:
                if op[0] == "ctx":
                    cur = op[1]
                elif op[0] == "split":
                    split[cur] = op[1]
                elif op[0] == "resize" or op[:2] in (("warm", 2), ("paircap", 50)):   # (these drop the visible list)
                    for key in [key for key in pruned_in if key[0] == cur]:
                        del pruned_in[key]
                elif op[0] == "recreate":                # (another buffer from here on)
                    for c in (0, 1):
                        history.pop((c, op[1]), None)
                        pruned_in.pop((c, op[1]), None)
            draws = by_frame[k]
            hows = {d["how"] for d in draws}
            for d in draws:
                self.hit[d["how"]] += 1
                if d["op"] == "buf":
                    key, mode = (d["ctx"], d["buf"]), _zmode(d["depth"])
                    history[key].append(d["how"])
                    if d["how"] == "pruned":
                        pruned_in[key] = mode
                    elif d["how"] == "cold":             # (a new schedule generation)
                        pruned_in.pop(key, None)
                    elif d["how"] == "reused":
                        self.hit["full list in another depth mode beside a visible list"] += pruned_in.get(key, mode) != mode
                if d["how"] != "pruned":
                    continue
                self.hit["pruned, LESS + write"] += d["depth"] == (True, True)
                self.hit["pruned, depth test off"] += not d["depth"][0]
                self.hit["pruned, RGBA"] += bool(alpha)
                self.hit["pruned, sharded"] += d["shard"] is not None
                nodepth = not any(op[0] in ("cleardepth", "shard", "resize") for op in ops)
                self.hit["pruned, no depth clear"] += nodepth
                # (a uniform colour clear stays pending: the pruned raster consumes it, with the per-tile fast clear)
                self.hit["pruned over a pending uniform colour clear"] += d["uniform"]
                self.hit["pruned over a pending uniform colour clear, no depth clear"] += d["uniform"] and nodepth
                self.hit["pruned over a pending uniform colour clear, sharded"] += d["uniform"] and d["shard"] is not None
                same_ctx = {e["buf"] for e in draws if e["op"] == "buf" and e["ctx"] == d["ctx"]}
                self.hit["pruned, two buffers in the frame"] += len(same_ctx) >= 2
                self.hit["pruned after unread frames"] += k > 0 and not frames[k - 1][1]
                n = got["counters"][k]
                tot = n.get("totals")
                if specs[d["buf"]][0] == "hidden" and split[d["ctx"]] == (64, 64) and d["ctx"] == cur and tot:
                    self.hit["hidden buffer pruned under split limits"] += tot["split"] > 2 and n["visible"] >= tot["split"]
            if "ordered" in hows and 0 < k < len(frames) - 1:
                around = [{d["how"] for d in by_frame[j]} & {"reused", "pruned"} for j in (k - 1, k + 1)]
                self.hit["ordered between two reused frames"] += all(around)
        for hist in history.values():
            first = hist.index("pruned") if "pruned" in hist else len(hist)
            later = [i for i in range(first, len(hist)) if hist[i] in BINS]
            self.hit["pruned, binned again, pruned again"] += bool(later) and "pruned" in hist[later[0]:]

    SMALL = ("cold", "warm", "loose", "reused", "pruned, LESS + write", "pruned, depth test off", "pruned, RGBA",
             "pruned, sharded", "pruned, no depth clear", "pruned, two buffers in the frame", "pruned after unread frames",
             "pruned, binned again, pruned again", "full list in another depth mode beside a visible list",
             "ordered between two reused frames", "hidden buffer pruned under split limits",
             "pruned over a pending uniform colour clear", "pruned over a pending uniform colour clear, no depth clear",
             "pruned over a pending uniform colour clear, sharded")
    # warm: neither loose nor reused -- at this size the inline binning, which the loose one meets here too
    LARGE = ("warm", "loose", "reused", "pruned", "pruned over a pending uniform colour clear")

    def check(self, want):
        print("reached:", dict(self.hit))
        missing = [w for w in want if not self.hit[w]]
        assert not missing, f"never reached: {missing} (reached: {dict(self.hit)})"


def _zmode(depth):
    """The rasters' depth modes: 0 no test, 1 LESS + write, 2 LESS without write."""
    return (1 if depth[1] else 2) if depth[0] else 0


def _compare(gpu, oracle, seq, reached=None):
    got = S.run(gpu, seq)
    want = S.run(oracle, seq)
    bad = S.mismatches(got, want)
    if bad or got["failures"] or got["error"]:
        print("failing sequence:", repr(seq))
        for k, n in enumerate(got["counters"]):
            print("  counters after frame", k, n)
        print("  draws:", [(d["frame"], d["ctx"], d["op"], d["buf"], d["how"]) for d in got["draws"]])
    assert not bad, (bad, seq)
    assert got["failures"] == 0 and got["error"] == "", (got["failures"], got["error"], seq)
    counted = [d for d in got["draws"] if d["counting"] and d["how"] == "pruned"]
    assert not counted, ("a batch whose fragments are counted was pruned", counted, seq)
    if reached is not None:
        reached.note(seq, got)
    return got


def test_random_sequences_match_oracle(gpu, oracle):
    reached = Reached()
    S.for_each_sequence("small", lambda seq: _compare(gpu, oracle, seq, reached))
    assert reached.sequences >= 40 and reached.frames >= 400, (reached.sequences, reached.frames)
    reached.check(Reached.SMALL)


def test_random_large_sequences_match_oracle(gpu, oracle):
    reached = Reached()
    sizes = []

    def visit(seq):
        sizes.append((S.triangle_count(seq[4][0]), len(seq[5])))
        _compare(gpu, oracle, seq, reached)

    S.for_each_sequence("large", visit)
    assert len(sizes) >= 2 and all(n >= 300000 and frames >= 8 for n, frames in sizes), sizes
    reached.check(Reached.LARGE)


# ---- fixed sequences -----------------------------------------------------------
NONUNI = [0.1, 0.2, 0.3, 0.9]
UNI = [0.2, 0.2, 0.2, 0.2]             # a uniform clear stays pending until a batch consumes it
CLEARS = [("clear", NONUNI), ("cleardepth", S.FULL)]
UNI_CLEARS = [("clear", UNI), ("cleardepth", S.FULL)]
A, B = ("buf", 0, "none", None), ("buf", 1, "none", None)
GOURAUD = ("gouraud", 600, 21, 12.0)
FLAT = ("flat", 500, 22, 12.0)
BLEND = ("blend", 300, 23, 12.0)


def _knobs(**kw):
    return dict(S.KNOBS_DEFAULT, **kw)


def fr(*ops, read=True):
    return (list(ops), read)


def reps(n, *pre, draws=(A,), clears=CLEARS, read=True):
    """n frames of the clears and the draws, the first one after `pre`."""
    return [fr(*(pre if k == 0 else ()), *clears, *draws, read=read) for k in range(n)]


def _moved(move):
    return fr(*CLEARS, ("buf", 0, move, None))


FIXED = {
    "prune_then_cleardepth_12345_without_colour_clear": (
        W, H, _knobs(), [GOURAUD], reps(5) + reps(2, clears=[("cleardepth", 12345)]) + reps(2)),
    "prune_then_frames_without_any_clear": (W, H, _knobs(), [GOURAUD], reps(5) + reps(4, clears=[]) + reps(2)),
    # LESS + write marks only over a depth cleared to 0xFFFFFFFF: not on frame 2 here, so frame 5 is not pruned
    "no_marking_frame_over_a_depth_cleared_to_another_value": (
        W, H, _knobs(), [GOURAUD],
        reps(5, clears=[("clear", NONUNI), ("cleardepth", 0x90000000)]) + reps(4)),
    "prune_under_less_write_then_depth_test_off_and_back": (
        W, H, _knobs(), [GOURAUD],
        reps(5) + reps(2, ("depthstate", False, False)) + reps(3, ("depthstate", True, True))),
    "marked_with_the_depth_test_off_then_less_write": (
        W, H, _knobs(), [GOURAUD],
        reps(5, ("depthstate", False, False)) + reps(2, ("depthstate", True, True)) + reps(2, ("depthstate", False, False))),
    "two_opaque_buffers_alternating_within_each_frame": (W, H, _knobs(), [GOURAUD, FLAT], reps(8, draws=(A, B))),
    "opaque_and_translucent_buffer_within_each_frame": (W, H, _knobs(), [GOURAUD, BLEND], reps(8, draws=(A, B))),
    "prune_then_shard_then_shard_off": (
        W, H, _knobs(), [GOURAUD], reps(5) + reps(5, ("shard", (2, 1))) + reps(5, ("shard", None))),
    "prune_then_ordered_colour_transform_and_back": (
        W, H, _knobs(), [GOURAUD],
        reps(5) + reps(1, ("ct", [0.9, 0.8, 0.7, 0.5])) + reps(4, ("ct", [0.9, 0.8, 0.7, 1.0]))),
    "prune_then_pair_capacity_override_and_back": (
        W, H, _knobs(), [GOURAUD], reps(5) + reps(1, ("paircap", 50)) + reps(5, ("paircap", 0))),
    "prune_then_recreate": (W, H, _knobs(), [GOURAUD], reps(5) + reps(5, ("recreate", 0, 77))),
    "moves_at_the_loose_boundary_after_a_prune": (
        W, H, _knobs(), [GOURAUD],
        reps(5) + [_moved("edge"), _moved("over")] + reps(2) + [_moved("sub"), _moved("scale")] + reps(2)),
    "prune_then_fragment_counting_for_two_frames": (
        W, H, _knobs(), [GOURAUD], reps(5) + reps(2, ("fragcount", True)) + reps(3, ("fragcount", False))),
    "hidden_buffer_under_split_limits_resized_and_back": (
        W, H, _knobs(split=(64, 64)), [("hidden", 11)],
        reps(5) + reps(5, ("resize", 64, 32)) + reps(5, ("resize", W, H))),
    "two_contexts_alternating_on_one_buffer": (
        W, H, _knobs(), [GOURAUD], [fr(("ctx", 0), *CLEARS, A, ("ctx", 1), *CLEARS, A) for _ in range(7)]),
    "unread_frames_then_read_ones": (W, H, _knobs(), [GOURAUD], reps(2) + reps(6, read=False) + reps(3)),
    "textured_buffer_opaque_then_rgba_texture_and_back": (
        W, H, _knobs(), [("tex", 400, 24, 12.0)],
        reps(5, draws=(("buf", 0, "none", "rgb"),)) + reps(1, draws=(("buf", 0, "none", "rgba"),)) +
        reps(3, draws=(("buf", 0, "none", "rgb"),))),
    "prune_then_uniform_clear_then_non_uniform_then_uniform": (
        W, H, _knobs(), [GOURAUD], reps(5) + reps(2, clears=UNI_CLEARS) + reps(2) + reps(2, clears=UNI_CLEARS)),
    "prune_over_uniform_clears_without_depth_clear_then_sharded": (
        W, H, _knobs(), [GOURAUD],
        reps(5, clears=UNI_CLEARS) + reps(3, clears=[("clear", UNI)]) + reps(5, ("shard", (2, 1)), clears=UNI_CLEARS) +
        reps(3, ("shard", None), clears=UNI_CLEARS)),
    "prune_over_uniform_clears_with_the_depth_test_off": (
        W, H, _knobs(), [GOURAUD],
        reps(5, ("depthstate", False, False), clears=UNI_CLEARS) + reps(3, clears=[("clear", UNI)]) + reps(2)),
    "frame_output_formats_over_pruned_frames_with_uniform_clears": (
        W, H, _knobs(), [GOURAUD],
        reps(5, clears=UNI_CLEARS) + reps(2, ("fmt", "rgb"), clears=UNI_CLEARS) + reps(2, ("fmt", "yuv420p"), clears=UNI_CLEARS) +
        reps(2, ("fmt", None), clears=UNI_CLEARS)),
    "frame_output_formats_over_pruned_frames": (
        W, H, _knobs(), [GOURAUD],
        reps(5) + reps(2, ("fmt", "rgb")) + reps(2, ("fmt", "yuv420p")) + reps(2, ("fmt", None))),
}


def _expect(name, got):
    """The sequence took the road it is named after.  The counts follow from
    the host code with every frame read: cold, warm binning, marking frame,
    then pruned (tests/test_visible_list_gpu.py)."""
    pruned = [n["pruned"] for n in got["counters"]]
    if name.startswith(("prune_", "moves_", "frame_output")):
        assert pruned[:5] == [0, 0, 0, 1, 2], pruned
    if "uniform" in name:
        over = [d["frame"] for d in got["draws"] if d["how"] == "pruned" and d["uniform"]]
        assert len(over) >= 4, over
    if name.startswith("no_marking"):
        assert pruned[:6] == [0] * 6 and pruned[-1] > 0, pruned
    if name.startswith("hidden"):
        assert pruned[4] == 2 and pruned[-1] > pruned[9] >= pruned[4], pruned
        n = got["counters"][-1]
        assert n["totals"]["split"] > 2 and n["visible"] >= n["totals"]["split"], n
    if name.startswith("two_contexts"):
        assert pruned[-1] >= 2 * 3, pruned               # each context prunes for itself
    if name.startswith("opaque_and_translucent"):
        assert pruned[-1] > 0 and "ordered" in {d["how"] for d in got["draws"]}, pruned
    if name.startswith("marked_with_the_depth_test_off"):
        assert pruned == [0, 0, 0, 1, 2, 2, 2, 3, 4], pruned


@pytest.mark.parametrize("alpha", [False, True], ids=["rgb", "rgba"])
@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_sequence(gpu, oracle, name, alpha):
    w, h, knobs, buffers, frames = FIXED[name]
    _expect(name, _compare(gpu, oracle, (w, h, alpha, knobs, buffers, frames)))
