"""Sequences of frames around repeat TriangleBuffer draws against the CPU
oracle, bit for bit: after every recorded frame the f64 framebuffer, the u32
depth and the u8 image or frame output (u8 image / YUV420P planes) of every
context, and the fragment counts while counting is on.

A sequence is plain data of tests/frame_seq.py's vocabulary, run by its one
interpreter on the library and on the oracle: the context lives for the whole
sequence, so a frame's pixels depend on what earlier frames left in the warm
schedule, the kept pair list, the visible list, the visible plan (work items
planned again from the kept counts) and the key cache (an unchanged draw shaded
from the keys one capture frame stored: stale keys would give an exact-looking
frame of another state) -- frames that accumulate
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

A batch shaded from the key cache is a pruned batch, in the library's counters
and here: its "how" is "pruned", so every "pruned, ..." state counts what it
counted before the key cache, and the "cached, ..." states count the cached
ones among them.  With every frame read the cache is reached by the sixth
unchanged frame (cold, warm binning, marking frame, pruned, capture frame,
cached); FIXED's "cached_" entries are the twins of its "prune_" ones with
seven such frames in front (lead), and CACHED holds the cached count after
every frame of each, derived from the host code (key_cache_step,
pruned_enqueue, reuse_enqueue, draw_free in nr_tri_free.hip).  None of the
listed states is out of the host code's reach.  One state depends on timing as
"pruned after unread frames" does: "cached after unread frames" needs the host
to have seen, by event queries alone, the marking frame, the key items' totals
and the capture frame complete while it ran ahead of unread frames.  It is
counted and printed with the others; whether it is also asserted is said at
Reached.SMALL.

No fault injection here (tests/test_warm_gpu.py, test_list_reuse_gpu.py and
test_visible_list_gpu.py inject faults): every sequence must end with no warm
failure and no latched error.

Running time, measured with --durations=0 on one MI355X (call phase; the commit before the key cache joined the
fuzz, then this one, in one session):
    test_random_sequences_match_oracle          before 1.91 s, 1.32 s, 1.56 s; now 1.56 s, 1.49 s, 1.56 s (1.46 s, 1.54 s)
                                                (64 sequences, 979 frames; before 841)
    test_random_large_sequences_match_oracle    before 1.16 s, 1.09 s, 1.13 s; now 1.29 s, 1.34 s, 1.34 s
                                                (3 sequences of 350 000 triangles, 40 frames; before 34)
    test_fixed_sequence, the slowest            before 0.02 s, 0.03 s, 0.02 s; now 0.03 s, 0.03 s, 0.03 s
                                                (cached_then_shard_then_shard_off, 21 frames)
Each is below 5 s and below three times the median before.  The example counts (frame_seq.SMALL_EXAMPLES = 64,
LARGE_EXAMPLES = 3) are above the floors of 40 small sequences with 400 frames and 2 large ones; if a test outgrows
the cap, lower the share of long sequences (frame_seq.make_small_seq), not the list of states.
"""
import collections

import hypothesis  # noqa: F401  (a missing package fails the module: these tests never skip)
import pytest

import frame_seq as S

pytestmark = pytest.mark.gpu

W, H = 200, 140            # 4 x 5 tiles, partial right and bottom tiles
BINS = ("cold", "warm", "loose")
# two of Reached's states, named in full
EMPTY_TILES = "cached with a frame output over a pending uniform clear to another colour, tiles without a kept pair"
STALE_DEPTH = "cached, then pruned but not cached over a depth nobody cleared to 0xFFFFFFFF, then cached again"


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
        keys_on = {0: knobs["keys"] == 0, 1: knobs["keys"] == 0}
        replan_on = {0: knobs["replan"] == 0, 1: knobs["replan"] == 0}
        # (context, buffer) -> how far along the roads named in SMALL the draws of that buffer are
        stale, resumed, regen, late = (collections.defaultdict(int) for _ in range(4))
        colour = {}
        for k, (ops, read) in enumerate(frames):
            mine = collections.defaultdict(list)         # context -> the frame's operations on it
            before = dict(colour)                        # context -> the last colour clear of the frames before
            for op in ops:
                if op[0] == "ctx":
                    cur = op[1]
                mine[cur].append(op)
                if op[0] == "clear":
                    colour[cur] = op[1]
                if op[0] == "keys":
                    keys_on[cur] = op[1] == 0
                    for key in [key for key in resumed if key[0] == cur]:
                        # cached (1), keys off (2), keys on again (3): the next draw of the buffer tells
                        resumed[key] = {(1, False): 2, (2, True): 3}.get((resumed[key], keys_on[cur]), resumed[key])
                elif op[0] == "replan":
                    replan_on[cur] = op[1] == 0
                if op[0] == "split":
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
                    self._roads(d, key, mine[d["ctx"]], keys_on, replan_on, stale, resumed, regen, late)
                if d["cached"]:
                    assert d["how"] == "pruned", d       # (a cached batch is a pruned batch)
                    self.hit["cached"] += 1
                    self.hit["cached, LESS + write"] += d["depth"] == (True, True)
                    self.hit["cached, depth test off"] += not d["depth"][0]
                    self.hit["cached, RGBA"] += bool(alpha)
                    self.hit["cached, sharded"] += d["shard"] is not None
                    self.hit["cached over a pending uniform colour clear"] += d["uniform"]
                    self.hit["cached over a non-uniform clear"] += d["written"]
                    others = [op for op in mine[d["ctx"]] if op[0] in ("rect", "circle", "tex", "host", "soup") or
                              (op[0] == "buf" and op[1] != d["buf"])]
                    self.hit["cached with primitives or another batch in the frame"] += bool(others)
                    self.hit["cached in the second context"] += d["ctx"] == 1
                    kt = got["counters"][k].get("keytotals") if d["ctx"] == cur else None
                    # (k_keys' empty items write their tiles of the frame output themselves: another colour than the
                    # frame before, or what is left there from that frame would do as well)
                    self.hit[EMPTY_TILES] += bool(
                        d["uniform"] and d["fmt"] and d["shard"] is None and kt and kt["tiles"] < kt["items"] and
                        before.get(d["ctx"]) != colour[d["ctx"]])
                    self.hit["cached after unread frames"] += k > 0 and not frames[k - 1][1]
                self.hit["replanned"] += d["replanned"]
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

    @staticmethod
    def _full_depth_clear(ops):
        """Do a context's operations of one frame leave its depth a clear to
        0xFFFFFFFF (a shard change and a resize do)?"""
        return any(op[:2] == ("cleardepth", S.FULL) or op[0] in ("shard", "resize") for op in ops)

    def _roads(self, d, key, ops, keys_on, replan_on, stale, resumed, regen, late):
        """One buffer draw along the roads that need more than one frame."""
        how, cached, c = d["how"], d["cached"], d["ctx"]
        # cached (1), pruned but not cached over a depth nobody cleared to 0xFFFFFFFF (2), cached again; no cold draw between
        if how == "cold":
            stale[key] = 0
        elif cached:
            self.hit[STALE_DEPTH] += stale[key] == 2
            stale[key] = 1
        elif (stale[key] == 1 and how == "pruned" and keys_on[c] and d["depth"] == (True, True) and
              not self._full_depth_clear(ops)):
            stale[key] = 2
        # cached (1), keys off (2) and on (3, both in note), and the first draw after that cached: no capture between,
        # because only pruned batches lie between and a pruned batch with the keys off leaves the key cache alone
        if resumed[key] == 3:
            self.hit["cached again after keys off and on without a capture between"] += cached
            resumed[key] = 0
        if cached:
            resumed[key] = 1
        elif how != "pruned":
            resumed[key] = 0
        # cached (1), a cold or warm draw of the buffer (2), cached again
        if cached:
            self.hit["cached after a new generation"] += regen[key] == 2
            regen[key] = 1
        elif regen[key] == 1 and how in ("cold", "warm"):
            regen[key] = 2
        # replanned (1), pruned under the schedule's items with the visible plan switched off (2), replanned again:
        # within one pruning, because only pruned (or ordered) batches lie between
        if how == "pruned" and d["replanned"]:
            self.hit["replanned, then replan off and on within one pruning"] += late[key] == 2
            late[key] = 1
        elif how == "pruned" and late[key] >= 1 and not replan_on[c]:
            late[key] = 2
        elif how not in ("pruned", "ordered"):
            late[key] = 0

    SMALL = ("cold", "warm", "loose", "reused", "pruned, LESS + write", "pruned, depth test off", "pruned, RGBA",
             "pruned, sharded", "pruned, no depth clear", "pruned, two buffers in the frame", "pruned after unread frames",
             "pruned, binned again, pruned again", "full list in another depth mode beside a visible list",
             "ordered between two reused frames", "hidden buffer pruned under split limits",
             "pruned over a pending uniform colour clear", "pruned over a pending uniform colour clear, no depth clear",
             "pruned over a pending uniform colour clear, sharded",
             "cached, LESS + write", "cached, depth test off", "cached, RGBA", "cached, sharded",
             "cached over a pending uniform colour clear", "cached over a non-uniform clear",
             STALE_DEPTH,
             "cached again after keys off and on without a capture between", "cached after a new generation",
             "cached with primitives or another batch in the frame", "replanned",
             "replanned, then replan off and on within one pruning", "cached in the second context",
             EMPTY_TILES,
             # (depends on timing; five consecutive runs of the test all reached it, each with the same count)
             "cached after unread frames")
    # warm: neither loose nor reused -- at this size the inline binning, which the loose one meets here too
    LARGE = ("warm", "loose", "reused", "pruned", "pruned over a pending uniform colour clear", "replanned", "cached")

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
UNI2 = [0.6, 0.6, 0.6, 0.6]
CLEARS = [("clear", NONUNI), ("cleardepth", S.FULL)]
UNI_CLEARS = [("clear", UNI), ("cleardepth", S.FULL)]
UNI2_CLEARS = [("clear", UNI2), ("cleardepth", S.FULL)]
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


def lead(*pre, **kw):
    """The seven unchanged frames that end shaded from the key cache twice: cold,
    warm binning, marking frame, pruned (the key items planned), capture frame,
    cached, cached -- the reps(5) of the entries above, two frames on."""
    return reps(7, *pre, **kw)


HIDDEN = ("hidden", 11)
PATCH = ("patch", 400, 25, 10.0)       # tiles without a kept pair: k_keys' empty items
RGB, RGBA = (("buf", 0, "none", "rgb"),), (("buf", 0, "none", "rgba"),)
TWO = [("ctx", 0), *CLEARS, A, ("ctx", 1), *CLEARS, A]
PRIMS = (("rect", [0.9, 0.2, 0.1, 0.5], [10.0, 10.0, 120.0, 90.0]), A,
         ("begin",), ("circle", [0.1, 0.8, 0.3, 0.6], [120.0, 70.0, 45.0]), ("end",))
OTHER_Z = [("clear", NONUNI), ("cleardepth", 0x80000000)]


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
    # ---- the key cache: the cached twins of the entries above (lead() in front; a tail of 2 frames where the
    # schedule generation survives the disturbance, of 7 where it ends), then the hand-offs of its own switches
    "cached_then_cleardepth_12345_without_colour_clear": (
        W, H, _knobs(), [GOURAUD], lead() + reps(2, clears=[("cleardepth", 12345)]) + reps(2)),
    "cached_then_frames_without_any_clear_then_clears": (W, H, _knobs(), [GOURAUD], lead() + reps(4, clears=[]) + reps(2)),
    "cached_under_less_write_then_depth_test_off_and_back": (
        W, H, _knobs(), [GOURAUD],
        lead() + reps(2, ("depthstate", False, False)) + reps(3, ("depthstate", True, True))),
    "cached_with_the_depth_test_off_then_less_write_and_back": (
        W, H, _knobs(), [GOURAUD],
        lead(("depthstate", False, False)) + reps(2, ("depthstate", True, True)) + reps(2, ("depthstate", False, False))),
    "cached_then_a_rect_and_a_recorded_circle_every_frame_without_colour_clear": (
        W, H, _knobs(), [GOURAUD], lead() + reps(3, draws=PRIMS, clears=[("cleardepth", S.FULL)]) + reps(2)),
    "cached_over_uniform_and_non_uniform_clears_alternating": (
        W, H, _knobs(), [GOURAUD], lead() + 4 * (reps(1, clears=UNI_CLEARS) + reps(1))),
    "cached_frame_output_formats_over_uniform_clears": (
        W, H, _knobs(), [GOURAUD],
        lead(clears=UNI_CLEARS) + reps(2, ("fmt", "rgb"), clears=UNI_CLEARS) + reps(2, ("fmt", "yuv420p"), clears=UNI_CLEARS) +
        reps(2, ("fmt", None), clears=UNI_CLEARS)),
    # (the colour changes with every frame: what the frame before left in the frame output would not do for a tile
    # without a kept pair, which k_keys' empty item has to write)
    "cached_frame_output_formats_over_uniform_clears_with_empty_tiles": (
        W, H, _knobs(), [PATCH],
        lead(clears=UNI_CLEARS) + reps(1, ("fmt", "rgb"), clears=UNI2_CLEARS) + reps(1, clears=UNI_CLEARS) +
        reps(1, ("fmt", "yuv420p"), clears=UNI2_CLEARS) + reps(1, clears=UNI_CLEARS) + reps(1, ("fmt", None), clears=UNI2_CLEARS) +
        reps(1, clears=UNI_CLEARS)),
    "cached_frame_output_formats_over_written_clears": (
        W, H, _knobs(), [GOURAUD],
        lead() + reps(2, ("fmt", "rgb")) + reps(2, ("fmt", "yuv420p")) + reps(2, ("fmt", None))),
    "cached_over_uniform_clears_without_depth_clear_then_sharded": (
        W, H, _knobs(), [GOURAUD],
        lead(clears=UNI_CLEARS) + reps(3, clears=[("clear", UNI)]) + reps(7, ("shard", (2, 1)), clears=UNI_CLEARS) +
        reps(7, ("shard", None), clears=UNI_CLEARS)),
    "cached_over_uniform_clears_with_the_depth_test_off": (
        W, H, _knobs(), [GOURAUD],
        lead(("depthstate", False, False), clears=UNI_CLEARS) + reps(3, clears=[("clear", UNI)]) + reps(2)),
    "cached_then_shard_then_shard_off": (
        W, H, _knobs(), [GOURAUD], lead() + reps(7, ("shard", (2, 1))) + reps(7, ("shard", None))),
    "cached_then_resized_smaller_and_back": (
        W, H, _knobs(split=(64, 64)), [HIDDEN], lead() + reps(7, ("resize", 64, 32)) + reps(7, ("resize", W, H))),
    "cached_then_recreate": (W, H, _knobs(), [GOURAUD], lead() + reps(7, ("recreate", 0, 77))),
    "cached_then_pair_capacity_override_and_back": (
        W, H, _knobs(), [GOURAUD], lead() + reps(1, ("paircap", 50)) + reps(7, ("paircap", 0))),
    # (a counted batch is binned and validated at once, and its binning becomes the schedule: draw_free's `exact`
    # leads to keep_binning and sched_capture, so fragment counting ends the generation too -- a tail of 7)
    "cached_then_fragment_counting_for_two_frames": (
        W, H, _knobs(), [GOURAUD], lead() + reps(2, ("fragcount", True)) + reps(7, ("fragcount", False))),
    "cached_then_ordered_colour_transform_and_back": (
        W, H, _knobs(), [GOURAUD],
        lead() + reps(1, ("ct", [0.9, 0.8, 0.7, 0.5])) + reps(4, ("ct", [0.9, 0.8, 0.7, 1.0]))),
    "two_contexts_alternating_on_one_buffer_cached": (W, H, _knobs(), [GOURAUD], [fr(*TWO) for _ in range(9)]),
    "unread_frames_then_read_ones_cached": (W, H, _knobs(), [GOURAUD], reps(2) + reps(6, read=False) + reps(7)),
    "textured_buffer_cached_then_rgba_texture_and_back": (
        W, H, _knobs(), [("tex", 400, 24, 12.0)], lead(draws=RGB) + reps(1, draws=RGBA) + reps(3, draws=RGB)),
    # ("over" is past the loose boundary: a new schedule under the moved transform, and another one back under the
    # first; the loose moves bin into a set of their own and leave the list, the visible list and the keys in place)
    "moves_at_the_loose_boundary_after_the_cache": (
        W, H, _knobs(), [GOURAUD],
        lead() + [_moved("edge"), _moved("over")] + reps(7) + [_moved("sub"), _moved("scale")] + reps(2)),
    "cached_then_keys_off_two_frames_then_on": (
        W, H, _knobs(), [GOURAUD], lead() + reps(2, ("keys", 2)) + reps(2, ("keys", 0))),
    # k_key_plan runs on a later batch of the pruned list than its first one
    "keys_off_until_pruned_then_on": (W, H, _knobs(keys=2), [GOURAUD], reps(5) + reps(4, ("keys", 0))),
    # the visible plan made on a cached batch, long after the pruning; the raster first runs under it when the keys go off
    "replan_off_until_cached_then_on_then_keys_off": (
        W, H, _knobs(split=(64, 64), replan=2), [HIDDEN], lead() + reps(2, ("replan", 0)) + reps(3, ("keys", 2))),
    # the slots are there from frame 4 on, but a LESS + write batch over a depth cleared to another value may not capture
    "slotted_but_depth_cleared_to_another_value_then_full": (
        W, H, _knobs(), [GOURAUD], reps(4) + reps(3, clears=OTHER_Z) + reps(3)),
}
LEAD = [0, 0, 0, 0, 0, 1, 2]           # the cached count over lead(), every frame read
NEW_GENERATION = [2, 2, 2, 2, 2, 3, 4]  # ... over 7 frames that start a schedule generation after it: cold, ..., cached, cached
# The cached counts after every frame (all read), from key_cache_step, pruned_enqueue, reuse_enqueue and draw_free:
# a batch is cached when the generation's keys are captured and seen (KeyStage::Cached), the keys are on, the batch is
# one of the pruned list (visible pruning on, no fragment counting, the list's depth mode) and visible_capture_ok
# holds -- the depth test off, or LESS + write over a depth still a pending clear to 0xFFFFFFFF.
CACHED = {
    "cached_then_cleardepth_12345_without_colour_clear": LEAD + [2, 2, 3, 4],
    "cached_then_frames_without_any_clear_then_clears": LEAD + [2, 2, 2, 2, 3, 4],
    # (the depth test off: not the list's mode, the full list, nothing marked or captured afresh)
    "cached_under_less_write_then_depth_test_off_and_back": LEAD + [2, 2, 3, 4, 5],
    "cached_with_the_depth_test_off_then_less_write_and_back": LEAD + [2, 2, 3, 4],
    # (primitives write colour only: the depth is still a pending clear when the buffer is drawn)
    "cached_then_a_rect_and_a_recorded_circle_every_frame_without_colour_clear": LEAD + [3, 4, 5, 6, 7],
    "cached_over_uniform_and_non_uniform_clears_alternating": LEAD + [3, 4, 5, 6, 7, 8, 9, 10],
    "cached_frame_output_formats_over_uniform_clears": LEAD + [3, 4, 5, 6, 7, 8],
    "cached_frame_output_formats_over_uniform_clears_with_empty_tiles": LEAD + [3, 4, 5, 6, 7, 8],
    "cached_frame_output_formats_over_written_clears": LEAD + [3, 4, 5, 6, 7, 8],
    "cached_over_uniform_clears_without_depth_clear_then_sharded": LEAD + [2, 2, 2] + NEW_GENERATION + [4, 4, 4, 4, 4, 5, 6],
    # (without the depth test every batch of the pruned list may be cached, whatever the depth holds)
    "cached_over_uniform_clears_with_the_depth_test_off": LEAD + [3, 4, 5, 6, 7],
    "cached_then_shard_then_shard_off": LEAD + NEW_GENERATION + [4, 4, 4, 4, 4, 5, 6],
    "cached_then_resized_smaller_and_back": LEAD + NEW_GENERATION + [4, 4, 4, 4, 4, 5, 6],
    "cached_then_recreate": LEAD + NEW_GENERATION,
    # (two counted frames, each a schedule of its own; then warm binning, marking, pruned, capture, cached x 3)
    "cached_then_fragment_counting_for_two_frames": LEAD + [2, 2] + [2, 2, 2, 2, 3, 4, 5],
    # (one ordered batch takes the binning set after the list's, not the list's: reused at once)
    "cached_then_ordered_colour_transform_and_back": LEAD + [2, 3, 4, 5, 6],
    "two_contexts_alternating_on_one_buffer_cached": [0, 0, 0, 0, 0, 2, 4, 6, 8],
    "textured_buffer_cached_then_rgba_texture_and_back": LEAD + [2, 3, 4, 5],
    "moves_at_the_loose_boundary_after_the_cache": LEAD + [2, 2] + NEW_GENERATION + [4, 4, 5, 6],
    "cached_then_keys_off_two_frames_then_on": LEAD + [2, 2, 3, 4],
    # (frame 5 plans the key items, frame 6 captures)
    "keys_off_until_pruned_then_on": [0, 0, 0, 0, 0, 0, 0, 1, 2],
    "replan_off_until_cached_then_on_then_keys_off": LEAD + [3, 4, 4, 4, 4],
    # (frame 3 plans, frame 4 allots the slots, frames 4-6 may not capture, frame 7 does)
    "slotted_but_depth_cleared_to_another_value_then_full": [0, 0, 0, 0, 0, 0, 0, 0, 1, 2],
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
    cached = [n["cached"] for n in got["counters"]]
    replanned = [n["replanned"] for n in got["counters"]]
    assert all(c <= p for c, p in zip(cached, pruned)), (cached, pruned)    # a cached batch is a pruned batch
    if name in CACHED:
        assert cached == CACHED[name], cached
    elif "cached" not in name:
        assert cached[:5] == [0] * 5, cached
    if name == "cached_then_pair_capacity_override_and_back":
        # the override drops the lists and frame 7 bins cold; whether its exact re-run leaves a schedule (frame 8 then
        # bins warm) or not (cold), no frame before 12 can be cached, and the last ones are
        assert cached[:11] == LEAD + [2] * 4 and cached[-1] > cached[-2] > 2, cached
    if name == "unread_frames_then_read_ones_cached":
        # every read frame advances at least one stage, so the last one is cached; how many before it depends on
        # how far the host ran ahead
        assert got["draws"][-1]["cached"] and cached[-1] > cached[-2], cached
    if name == "cached_then_fragment_counting_for_two_frames":
        assert [d["how"] for d in got["draws"]][7:11] == ["cold", "cold", "warm", "reused"], got["draws"][7:11]
    if name == "replan_off_until_cached_then_on_then_keys_off":
        # the plan is made on frame 7, a cached batch; frames 9-11 rasterise under it
        assert replanned == [0] * 7 + [1, 2, 3, 4, 5], replanned
        assert pruned == [0, 0, 0] + list(range(1, 10)), pruned
        assert got["counters"][6]["vplan"] is None and got["counters"][-1]["vplan"]["items"] > 0, got["counters"][-1]
    if name == "cached_then_resized_smaller_and_back":
        assert replanned == pruned and pruned[-1] == 3 * 4, (replanned, pruned)   # (split tiles: every pruned batch re-planned)
        n = got["counters"][-1]
        assert n["totals"]["split"] > 2 and n["visible"] >= n["totals"]["split"] and n["keytotals"]["tiles"] > 0, n
    if name.endswith("with_empty_tiles"):
        kt = got["counters"][-1]["keytotals"]
        assert 0 < kt["tiles"] < kt["items"] == 4 * 5, kt
    if name == "slotted_but_depth_cleared_to_another_value_then_full":
        assert pruned == [0, 0, 0, 1, 2, 3, 4, 5, 6, 7], pruned
        assert got["counters"][6]["keytotals"] is not None, got["counters"][6]
    if name == "keys_off_until_pruned_then_on":
        assert got["counters"][4]["keytotals"] is None and got["counters"][5]["keytotals"] is not None, got["counters"]


@pytest.mark.parametrize("alpha", [False, True], ids=["rgb", "rgba"])
@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_sequence(gpu, oracle, name, alpha):
    w, h, knobs, buffers, frames = FIXED[name]
    _expect(name, _compare(gpu, oracle, (w, h, alpha, knobs, buffers, frames)))
