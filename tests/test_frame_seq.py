"""The sequence vocabulary on the oracle alone (no GPU): the sequences its
strategies generate -- exactly the examples tests/test_seq_fuzz_gpu.py runs --
hold what that test is there for, and the interpreter is self-consistent."""
import numpy as np
import pytest

import frame_seq as S
import scenes
import test_seq_fuzz_gpu as G


def _examples(kind):
    seqs = []
    S.for_each_sequence(kind, seqs.append)
    return seqs


@pytest.fixture(scope="module")
def small():
    return _examples("small")


@pytest.fixture(scope="module")
def large():
    return _examples("large")


def test_the_generator_is_deterministic(small, large):
    assert repr(_examples("small")) == repr(small)
    assert repr(_examples("large")) == repr(large)
    assert len({repr(s) for s in small}) == len(small)


def test_small_sequences_hold_every_operation_and_hand_off(small):
    assert len(small) >= 40 and sum(len(s[5]) for s in small) >= 400
    held = [S.describe(s) for s in small]
    for W, H, alpha, knobs, specs, frames in small:
        assert (W, H) in ((200, 140), (64, 32), (1, 58)) and 8 <= len(frames) <= 24 and 1 <= len(specs) <= 3
        assert all(200 <= S.triangle_count(spec) <= 3000 for spec in specs)
    assert {(s[0], s[1]) for s in small} == {(200, 140), (64, 32), (1, 58)}
    ops = set().union(*[d["ops"] for d in held])
    assert ops == set(S.ALL_OPS), (sorted(set(S.ALL_OPS) - ops), sorted(ops - set(S.ALL_OPS)))
    assert set().union(*[d["kinds"] for d in held]) == set(S.BUFFER_KINDS)
    assert set().union(*[d["moves"] for d in held]) == set(S.MOVES)      # each after a repeat of the same buffer
    for name in S.KNOB_OPS:                                                # every knob flipped mid-sequence, both ways
        values = {repr(op[1]) for s in small for ops, _ in s[5] for op in ops if op[0] == name}
        assert len(values) >= 2, (name, values)
    assert {op[1] for s in small for ops, _ in s[5] for op in ops if op[0] == "fmt"} == {None, "rgb", "yuv420p"}
    assert any(d["unclear"] >= 4 for d in held), "no colour or depth clear for 4 frames"
    # uniform colour clears (they stay pending in the library) and others (written), each after a repeat
    for kind in ("uniform", "other"):
        assert sum(kind in d["clears"] for d in held) >= len(small) // 4, kind
    assert sum(d["clears"] == {"uniform", "other"} for d in held) >= 5, "both kinds in one sequence"
    assert any(d["two"] for d in held), "two different buffers in one frame"
    assert any(s[2] for s in small) and any(not s[2] for s in small), "alpha"
    assert any(d["shard_mid"] for d in held), "a shard change mid-sequence"
    assert any(d["unread"] >= 4 for d in held), "4 unread frames after a repeat"
    # runs of unchanged repeats, long enough for the visible list: 5 frames in a row with the same operations
    runs = [S._longest([a[0] == b[0] for a, b in zip(s[5], s[5][1:])]) + 1 for s in small]
    assert sum(n >= 5 for n in runs) >= len(small) // 2, runs
    # ... and for the key cache: six unchanged read frames reach it (cold, warm, marking, pruned, capture, cached),
    # a seventh is shaded from it once more; cached, then disturbed, then room to be cached again
    quiet = [S.quiet_runs(s[5]) for s in small]
    assert sum(any(n >= 7 for _, n in q) for q in quiet) >= (len(small) + 3) // 4, quiet
    again = [any(n >= 6 and len(s[5]) - (k + n + 1) >= 6 for k, n in q) for s, q in zip(small, quiet)]
    assert sum(again) >= 8, again
    assert sum(len(s[5]) >= 18 for s in small) >= len(small) // 5, "the long flavour"


def test_large_sequences_reach_the_inline_binning_size(large):
    assert len(large) >= 2
    allowed = {"clear", "cleardepth", "depthstate", "buf", "resize"}
    for W, H, alpha, knobs, specs, frames in large:
        assert (W, H) == (640, 400) and len(specs) == 1 and len(frames) >= 8
        assert S.triangle_count(specs[0]) >= 300000 and len(S.buffer_arrays(specs[0], W, H)[0]) == S.triangle_count(specs[0])
        assert {op[0] for ops, _ in frames for op in ops} <= allowed
        assert knobs == S.KNOBS_DEFAULT
        # the visible plan (the schedule has split tiles) and the key cache: six unchanged read frames first
        assert S.quiet_runs(frames)[0][0] == 0 and S.quiet_runs(frames)[0][1] >= 6, S.quiet_runs(frames)
        # after a repeat: a loose move, and a depth-mode switch or a resize and back to the first size
        held = S.describe((W, H, alpha, knobs, specs, frames))
        assert held["moves"] & {"sub", "edge"}, held["moves"]
        sizes = [op[1:] for ops, _ in frames[4:] for op in ops if op[0] == "resize"]
        switched = any(op[0] == "depthstate" for ops, _ in frames[4:] for op in ops)
        assert switched or (len(sizes) >= 2 and (W, H) in sizes[1:]), (sizes, switched)
    ops = {op[0] for _, _, _, _, _, frames in large for fr, _ in frames for op in fr}
    assert {"depthstate", "resize"} <= ops, ops
    assert any(len(set(op[1])) == 1 for s in large for fr, _ in s[5] for op in fr if op[0] == "clear"), "a uniform clear"


def test_generated_and_fixed_sequences_run_on_the_oracle(oracle, small):
    fixed = [(w, h, alpha, knobs, bufs, frames) for w, h, knobs, bufs, frames in G.FIXED.values() for alpha in (False, True)]
    for seq in small + fixed:
        out = S.run(oracle, seq)
        frames = seq[5]
        read = [k for k, (_, r) in enumerate(frames) if r or k == len(frames) - 1]
        assert sorted({r["k"] for r in out["records"]}) == read
        assert all(np.isfinite(r["f64"]).all() for r in out["records"])
        assert out["draws"] == [] and out["counters"] == []
    a = S.run(oracle, small[1])
    assert S.mismatches(a, S.run(oracle, small[1])) == []
    assert S.mismatches(a, S.run(oracle, small[2])) != []


CLEARS = [("clear", [0.1, 0.2, 0.3, 0.9]), ("cleardepth", S.FULL)]
SELF_CONTAINED = [      # every frame starts with both clears and sets the state it draws under
    CLEARS + [("depthstate", True, True), ("ct", [1.0, 1.0, 1.0, 1.0]), ("buf", 0, "none", None), ("buf", 1, "sub", "rgb")],
    CLEARS + [("depthstate", False, False), ("ct", [0.9, 0.8, 0.7, 1.0]), ("buf", 1, "far", "rgba"),
              ("rect", [0.9, 0.2, 0.1, 0.5], [10.0, 10.0, 120.0, 90.0]), ("buf", 2, "none", None)],
    CLEARS + [("depthstate", True, False), ("ct", [1.0, 1.0, 1.0, 0.5]), ("buf", 0, "scale", None), ("soup", 5),
              ("circle", [0.1, 0.8, 0.3, 0.6], [120.0, 70.0, 45.0]), ("host", 3, None)],
    CLEARS + [("depthstate", True, True), ("ct", [1.0, 1.0, 1.0, 1.0]), ("buf", 3, "edge", None),
              ("tex", "rgba", [30.0, 20.0, 100.0, 80.0]), ("buf", 0, "over", None)],
]
SPECS = [("gouraud", 300, 1, 12.0), ("tex", 200, 2, 12.0), ("blend", 200, 3, 12.0), ("hidden", 4)]


@pytest.mark.parametrize("alpha", [False, True])
def test_a_sequence_of_self_contained_frames_is_its_frames_alone(oracle, alpha):
    frames = [(ops, True) for ops in SELF_CONTAINED + SELF_CONTAINED[::-1]]
    whole = S.run(oracle, (200, 140, alpha, S.KNOBS_DEFAULT, SPECS, frames))["records"]
    assert len(whole) == len(frames)
    for k, frame in enumerate(frames):
        alone, = S.run(oracle, (200, 140, alpha, S.KNOBS_DEFAULT, SPECS, [frame]))["records"]
        for what in ("f64", "depth", "u8"):
            assert scenes.bits_equal(whole[k][what], alone[what]), (k, what, scenes.first_mismatch(whole[k][what], alone[what]))
    assert not scenes.bits_equal(whole[0]["f64"], whole[1]["f64"])
