"""Whole frames that mix every draw kind, on every raster path, against the
CPU oracle bit for bit: f64 framebuffer, u32 depth, u8 readback, the frame
output (u8 image / YUV420P planes) and every mid-frame probe.

A frame is plain data of tests/frame_ops.py's vocabulary (colour soups from
host arrays, TriangleBuffers and device arrays; textured soups, with q too;
indexed meshes with update_positions, instanced with tints, lit, lit and
instanced; the five sticky states those draws read -- near plane, cull mode,
mesh perspective, texture filter, lights; primitives, textures, pixels;
snapshots of the frame and of an auxiliary context; state; probes; command
recording; the frame output; the testing knobs of the rasters), run by its one
interpreter on the library and on the oracle.  frame_ops.py states how the oracle, which has no
textured draw, mesh, buffer or recording, runs each operation;
tests/test_frame_ops.py checks the lowerings and that the generated frames
are worth running, on exactly the examples drawn here.

tests/frame_anim.py extends the vocabulary and the interpreter by the texture
wrap (the sixth sticky state), modulated textured soups, textured colour
meshes, unlit and lit, and meshes posed, morphed or both between their draws,
from the main or the auxiliary context; a run on the library then also
compares the arrays the pose kernels left in every posed mesh.

Six property tests draw the frames (hypothesis, derandomized: the "small" and
"large" examples, which never change, the "small-state" and "large-state"
ones, which add the states and the draws that read them, and the "small-anim"
and "large-anim" ones of frame_anim.py); the fixed
sequences below them are the hand-offs between kinds named one by one, in the
same data, so that a failing fuzz frame (printed with its knobs) can be added
as one more entry of FIXED.

Running time, measured with --durations on one MI355X (call phase, two runs):
    tests/test_fuzz_gpu.py::test_random_frames_match_oracle         1.74 s, 1.62 s (400 examples)
    tests/test_fuzz_gpu.py::test_random_large_frames_match_oracle   1.03 s, 1.01 s (40 examples)
    test_random_mixed_frames_match_oracle                           0.83 s (200 examples)
    test_random_mixed_large_frames_match_oracle                     0.62 s (50 examples)
The example counts (frame_ops.SMALL_EXAMPLES = 200, LARGE_EXAMPLES = 50) are above the floor of 150 small and 20
large frames and keep each test shorter than its old counterpart; each fixed sequence takes about 10 ms.
The state frames beside the frames above, in one session each (call phase, two sessions):
    test_random_mixed_frames_match_oracle                           1.40 s, 1.15 s (200 examples)
    test_random_state_frames_match_oracle                           2.08 s, 1.76 s (200 examples, up to 18 operations)
    test_random_mixed_large_frames_match_oracle                     0.74 s, 0.60 s (50 examples)
    test_random_large_state_frames_match_oracle                     0.75 s, 0.72 s (50 examples)
The anim frames beside all of the above (call phase; this module alone, then the whole GPU suite, where the large
tests were below the twelve slowest that were listed):
    test_random_state_frames_match_oracle                           1.80 s, 1.74 s (200 examples)
    test_random_anim_frames_match_oracle                            2.18 s, 2.14 s (200 examples, up to 18 operations)
    test_random_large_state_frames_match_oracle                     0.74 s (50 examples)
    test_random_large_anim_frames_match_oracle                      0.96 s (50 examples)
"""
import hypothesis  # noqa: F401  (a missing package fails the module: these tests never skip)
import pytest

import frame_anim as A
import frame_ops as F

pytestmark = pytest.mark.gpu

W, H = 200, 140            # 4 x 5 tiles, partial right and bottom tiles
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


class Reached:
    """What the frames of one property test reached on the GPU."""

    def __init__(self):
        self.paths = set()          # (triangle kind, raster path)
        self.warm = 0
        self.over_cap = 0           # frames under set_pair_capacity_override(50) with a batch of more pairs
        self.changed_over_cap = 0   # ... where one of the five sticky states changed before the next synchronisation
        self.posed_paths = set()    # raster paths of the draws of posed or morphed meshes
        self.posed_over_cap = 0     # ... where a mesh was posed between two draws of it, the first behind such a batch
        self.wrap_over_cap = 0      # ... where the wrap changed before the next synchronisation
        self.frames = 0

    def note(self, frame, got):
        self.frames += 1
        self.paths |= {(kind, path) for kind, path, _ in got["batches"]}
        self.warm += got["warm"] > 0
        self.over_cap += frame[3]["paircap"] == 50 and any(pairs > 50 for _, _, pairs in got["batches"])
        self.changed_over_cap += frame[3]["paircap"] == 50 and got["changed_over_cap"] > 0
        self.posed_paths |= got.get("posed_paths", set())
        self.posed_over_cap += frame[3]["paircap"] == 50 and got.get("posed_over_cap", 0) > 0
        self.wrap_over_cap += frame[3]["paircap"] == 50 and got.get("wrap_over_cap", 0) > 0

    def check(self, states=False, anim=False):
        kinds = ("colour", "textured", "mesh") + (("instanced", "lit") if states else ()) + (("modulated",) if anim else ())
        want = {(k, p) for k in kinds for p in ("order-free", "ordered")}
        assert want <= self.paths, f"never reached: {sorted(want - self.paths)}"
        assert self.warm > 0, "no frame with a warm batch"
        assert self.over_cap > 0, "no frame overflowed the pair capacity of 50"
        if states:
            assert self.changed_over_cap > 0, "no sticky state changed while an overflowed batch could be pending"
        if anim:
            assert {"order-free", "ordered"} <= self.posed_paths, f"posed meshes drawn on {sorted(self.posed_paths)} only"
            assert self.posed_over_cap > 0, "no mesh posed between two draws of it behind an overflowed batch"
            assert self.wrap_over_cap > 0, "the wrap never changed while an overflowed batch could be pending"
        print("reached:", sorted(self.paths), "frames", self.frames, "warm", self.warm, "over_cap", self.over_cap,
              "changed_over_cap", self.changed_over_cap, "posed paths", sorted(self.posed_paths),
              "posed_over_cap", self.posed_over_cap, "wrap_over_cap", self.wrap_over_cap)


def _compare(gpu, oracle, frame, reached=None, run=F.run):
    got = run(gpu, frame)
    want = run(oracle, frame)
    bad = F.mismatches(got, want)
    if bad:
        print("mismatching frame:", repr(frame))
    assert not bad, (bad, frame)
    assert [b[0] for b in got["batches"]] == [b[0] for b in want["batches"]]
    assert got["counts"] == want["counts"]
    if reached is not None:
        reached.note(frame, got)
    return got


def test_random_mixed_frames_match_oracle(gpu, oracle):
    reached = Reached()
    F.for_each_frame("small", lambda fr: _compare(gpu, oracle, fr, reached))
    assert reached.frames >= 150
    reached.check()


def test_random_mixed_large_frames_match_oracle(gpu, oracle):
    reached = Reached()
    F.for_each_frame("large", lambda fr: _compare(gpu, oracle, fr, reached))
    assert reached.frames >= 20
    reached.check()


def test_random_state_frames_match_oracle(gpu, oracle):
    reached = Reached()
    F.for_each_frame("small-state", lambda fr: _compare(gpu, oracle, fr, reached))
    assert reached.frames >= 150
    reached.check(states=True)


def test_random_large_state_frames_match_oracle(gpu, oracle):
    reached = Reached()
    F.for_each_frame("large-state", lambda fr: _compare(gpu, oracle, fr, reached))
    assert reached.frames >= 20
    reached.check(states=True)


def test_random_anim_frames_match_oracle(gpu, oracle):
    reached = Reached()
    A.for_each_frame("small-anim", lambda fr: _compare(gpu, oracle, fr, reached, A.run))
    assert reached.frames >= 150
    reached.check(states=True, anim=True)


def test_random_large_anim_frames_match_oracle(gpu, oracle):
    reached = Reached()
    A.for_each_frame("large-anim", lambda fr: _compare(gpu, oracle, fr, reached, A.run))
    assert reached.frames >= 20
    reached.check(states=True, anim=True)


# ---- fixed sequences -----------------------------------------------------------
def _knobs(**kw):
    return dict(F.KNOBS_OFF, **kw)


RGB_TEX = (37, 23, 3, "f64", 5, None)
RGBA_TEX = (16, 9, 4, "u8", 6, None)
GOURAUD_MESH = ("c", "model", 8, 12, 3, True, False)
TWO_TILES = (0.3, 0.0, 0.0, 0.2, 5.0, 3.0)     # the frame onto its top-left 60 x 28 pixels
BG = ("clear", [0.3, 0.6, 0.9, 2.7])           # set_color(0.1, 0.2, 0.3, 0.9): non-uniform, alpha on RGB


def _kinds_in_one_depth_buffer(test, write):
    return (_knobs(), dict(texs=[RGB_TEX, RGBA_TEX], bufs=[], meshes=[GOURAUD_MESH]),
            [("depthstate", test, write),
             ("tri", "host", 150, 11, 40.0, False, False), ("ttri", "host", 150, 12, 40.0, "const", ("res", 0)),
             ("tri", "host", 100, 13, 40.0, True, True), ("ttri", "host", 100, 14, 40.0, "const", ("res", 1)),
             ("mesh", 0, 1, ("res", 0))])


def _overflow_then_clears(first, fmt):
    res = dict(texs=[RGB_TEX], bufs=[], meshes=[("c", "screen", 10, 10, 4, True, False)])
    return (_knobs(paircap=50, fmt=fmt), res,
            [first, ("cleardepth", 0xFFFFFFFF), BG, ("rect", [0.9, 0.2, 0.1, 0.5], [10.0, 10.0, 120.0, 90.0]),
             ("tri", "host", 60, 22, 6.0, True, False)])


def _fast_clear(batch1, batch2):
    res = dict(texs=[RGB_TEX, (9, 13, 4, "u8", 8, None)], bufs=[], meshes=[("c", "screen", 6, 8, 5, True, False)])
    return (_knobs(), res,
            [BG, ("cleardepth", 0xFFFFFFF0), ("transform", TWO_TILES), batch1, ("transform", IDENT),
             ("tex", ("res", 1), [-5.0, -4.0, 210.0, 150.0]), ("getcolor", 190.0, 130.0),
             ("transform", TWO_TILES), batch2, ("readdepth",)])


LIT_MESH = ("l", "model", 8, 12, 3, True, False)          # 192 triangles
TU_MESH = ("tu", "model", 40, 7, 0.3)


def _states_survive(fmt):
    res = dict(texs=[RGB_TEX], bufs=[], meshes=[LIT_MESH, TU_MESH])
    return (_knobs(fmt=fmt, coop=2), res,
            [("lights", 4, 8), ("near", 0.5), ("cull", 2), ("mpersp", True), ("filter", 1),
             ("save", [0.0] * 4), ("resize", 150, 100), ("restore", [0.0] * 4), BG,
             ("meshi", 1, 3, 31, None, "host"), ("lmesh", 0, 2, 12), ("lmesh2", 0, 1, None, 13),
             ("lmeshi", 0, 3, 32, "alpha", "dev8"), ("ptri", "dev", 80, 33, 40.0, ("res", 0))])


def _tinted_lit_between_instanced(test, write):
    return (_knobs(), dict(texs=[], bufs=[], meshes=[LIT_MESH]),
            [("depthstate", test, write), ("lights", 4, 3), ("meshi", 0, 4, 41, "opaque", "host"),
             ("lmeshi", 0, 4, 42, "alpha", "host"), ("meshi", 0, 4, 43, None, "dev")])


TL_MESH = ("tl", "model", 150, 4, 0.6)          # (opaque colours, an RGB texture)
TC_MESH = ("tc", "model", 60, 7, 0.6)
RIG = (0, 5, 41, True, 0)
MORPH = (0, 5, 43, True)
_MOD = ("mtri", "host", 150, 52, 40.0, "flat", False, None, ("res", 0))
_MOD_BLENDED = ("mtri", "dev8", 100, 53, 40.0, "gouraud", True, "pow2", ("pow2", 3, 4))


def _posed_as_every_draw_kind(test, write):
    res = dict(texs=[RGB_TEX], bufs=[], meshes=[LIT_MESH], rigs=[RIG], morphs=[MORPH])
    return (_knobs(), res,
            [("depthstate", test, write), ("near", 0.5), ("cull", 2), ("lights", 4, 3), ("pose", 0, 7, "host", "main"),
             ("tri", "host", 150, 11, 40.0, False, False), ("mesh", 0, 2, ("res", 0)), ("meshi", 0, 3, 31, "alpha", "host"),
             _MOD, ("lmesh", 0, 2, 12), ("lmeshi", 0, 3, 32, "opaque", "dev")])


def _six_states_survive(fmt):
    res = dict(texs=[RGB_TEX], bufs=[], meshes=[LIT_MESH, TU_MESH, TC_MESH])
    return (_knobs(fmt=fmt, coop=2), res,
            [("lights", 4, 8), ("near", 0.5), ("cull", 2), ("mpersp", True), ("filter", 1), ("wrap", 1, 2),
             ("save", [0.0] * 4), ("resize", 150, 100), ("restore", [0.0] * 4), BG,
             ("meshi", 1, 3, 31, None, "host"), ("lmesh", 0, 2, 12), ("mesh", 2, 2, ("res", 0)),
             ("ttri", "dev", 80, 33, 40.0, "tiled", ("res", 0)), _MOD])


_TEXTURED = ("ttri", "host", 300, 21, 40.0, "const", ("res", 0))
_TEXTURED_SMALL = ("ttri", "host", 80, 23, 6.0, "const", ("res", 0))
_MESH = ("mesh", 0, 0, ("res", 0))

FIXED = {
    "kinds_in_one_depth_buffer_test_write": _kinds_in_one_depth_buffer(True, True),
    "kinds_in_one_depth_buffer_test_only": _kinds_in_one_depth_buffer(True, False),
    "kinds_in_one_depth_buffer_depth_off": _kinds_in_one_depth_buffer(False, False),
    "six_buffer_batches_rotate_the_binning_sets": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[("c", 120, 31, 40.0, True, False), ("t", 120, 32, 40.0, "const")],
                                 meshes=[]),
        [("buf", 0, ("res", 0)), ("translate", [0.7, 0.3, 0.0, 0.0]), ("buf", 1, ("res", 0)),
         ("translate", [-0.7, -0.3, 0.0, 0.0]), ("buf", 0, ("res", 0)), ("translate", [0.7, 0.3, 0.0, 0.0]),
         ("buf", 1, ("res", 0)), ("translate", [-0.7, -0.3, 0.0, 0.0]), ("buf", 0, ("res", 0)),
         ("translate", [0.7, 0.3, 0.0, 0.0]), ("buf", 1, ("res", 0))]),
    "overflowing_textured_batch_then_clears": _overflow_then_clears(_TEXTURED, None),
    "overflowing_mesh_then_clears": _overflow_then_clears(_MESH, None),
    "overflowing_textured_batch_then_clears_frame_output": _overflow_then_clears(_TEXTURED, "rgb"),
    "overflowing_mesh_then_clears_frame_output": _overflow_then_clears(_MESH, "yuv420p"),
    # the state a later re-run must not pick up: colour transform and depth state changed while the batch is pending
    "rerun_keeps_the_colour_transform_and_depth_state_of_its_batch": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[], meshes=[("c", "screen", 10, 10, 4, True, False)]),
        [_TEXTURED, ("ct", [1.5, 2.4, 0.9, 3.0]), ("depthstate", False, False),
         ("rect", [0.9, 0.2, 0.1, 0.5], [10.0, 10.0, 120.0, 90.0]), ("ct", [2.7, 1.2, 2.1, 3.0]), ("depthstate", True, True),
         _MESH, ("ct", [0.6, 0.6, 2.4, 3.0]), ("depthstate", True, False), ("tri", "host", 200, 25, 40.0, True, False),
         ("ct", [3.0, 3.0, 3.0, 1.5]), ("readdepth",)]),
    "fast_clear_textured_batches_in_two_tiles": _fast_clear(_TEXTURED_SMALL, ("ttri", "host", 80, 24, 6.0, "const", ("res", 0))),
    "fast_clear_meshes_in_two_tiles": _fast_clear(_MESH, ("mesh", 0, 1, ("res", 0))),
    "recorded_primitives_between_batches": (
        _knobs(), dict(texs=[RGB_TEX, RGBA_TEX], bufs=[], meshes=[GOURAUD_MESH]),
        [("begin",), ("rect", [0.9, 0.2, 0.1, 0.5], [10.0, 10.0, 120.0, 90.0]), ("tex", ("res", 1), [30.0, 20.0, 100.0, 80.0]),
         ("ttri", "host", 120, 41, 40.0, "const", ("res", 0)), ("circle", [0.1, 0.8, 0.3, 0.6], [120.0, 70.0, 45.0, 0.0]),
         ("mesh", 0, 1, ("res", 0)), ("stex", ("res", 1), [60.0, 30.0, 90.0, 70.0], [0.2, 0.7, 0.1, 0.9]), ("flush",),
         ("tri", "host", 120, 42, 40.0, True, False), ("end",)]),
    # found by the fuzz: the colour entry points left the recorded list queued, so it ran after their batch
    "recorded_fill_before_colour_batches": (
        _knobs(record=True), dict(texs=[], bufs=[("c", 60, 44, 40.0, True, False)], meshes=[]),
        [("fill", [0.66, 0.12, 0.95, 0.4]), ("tri", "host", 60, 43, 40.0, True, False),
         ("rect", [0.9, 0.2, 0.1, 0.5], [10.0, 10.0, 120.0, 90.0]), ("tri", "dev", 60, 45, 40.0, False, False),
         ("circle", [0.1, 0.8, 0.3, 0.6], [120.0, 70.0, 45.0, 0.0]), ("buf", 0, ("tiny", 1, 3)),
         ("fill", [0.2, 0.9, 0.4, 0.3]), ("tri", "dev8", 60, 46, 40.0, True, True)]),
    "shared_frame_texture_survives_the_rerun": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[], meshes=[]),
        [("grd", [0.9, 0.1, 0.4, 1.0], [0.0, 0.0, 200.0, 140.0]), ("tri", "host", 40, 51, 40.0, True, False),
         ("ttri", "host", 300, 52, 40.0, "const", ("snap", "main", True)), ("begin",),
         ("tex", ("snap", "main", True), [20.0, 10.0, 90.0, 60.0]), ("end",)]),
    "texture_shared_from_a_recording_context": (
        _knobs(record=True), dict(texs=[], bufs=[], meshes=[]),
        [("aux", "rect", [0.9, 0.2, 0.1, 1.0], [3.0, 2.0, 10.0, 8.0]), ("snap", "aux", True),
         ("aux", "clear", [0.2, 0.7, 0.4, 1.0], [0.0, 0.0, 0.0, 0.0]),
         ("aux", "circle", [0.1, 0.3, 0.9, 0.8], [12.0, 9.0, 7.0, 0.0]), ("aux", "rect", [0.9, 0.9, 0.1, 0.5], [1.0, 1.0, 5.0, 20.0]),
         ("ttri", "host", 150, 61, 40.0, "const", ("snap", "aux", True))]),
    "moved_mesh_warm_buffer_resize": (
        _knobs(), dict(texs=[RGB_TEX], bufs=[("c", 120, 71, 40.0, True, False)], meshes=[GOURAUD_MESH]),
        [("mesh2", 0, 1, ("res", 0), 72), ("buf2", 0, ("res", 0), 0.0), ("resize", 150, 100),
         ("mesh", 0, 1, ("res", 0)), ("buf", 0, ("res", 0))]),
    # the mesh staging regrown by a larger draw, then reused by a smaller one, while the lit draw that filled it
    # first is re-run; lights, near plane and cull mode change while that draw is pending
    "lit_rerun_after_the_staging_regrows_and_shrinks": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[], meshes=[LIT_MESH, ("c", "model", 10, 10, 4, True, False), TU_MESH]),
        [("lights", 4, 3), ("lmesh", 0, 1, 12), ("lights", 5, 8), ("near", 0.5), ("cull", 1),
         ("meshi", 1, 5, 31, "opaque", "host"), ("mesh", 2, 2, ("res", 0))]),
    "recorded_filter_and_perspective_flushed_once": (
        _knobs(record=True), dict(texs=[RGB_TEX], bufs=[("t", 120, 32, 40.0, "const")], meshes=[TU_MESH]),
        [("buf", 0, ("res", 0)), ("filter", 1), ("mpersp", True), ("mesh", 0, 0, ("res", 0)), ("filter", 0),
         ("ptri", "host", 100, 33, 40.0, ("res", 0))]),
    "states_survive_save_resize_restore_clear": _states_survive("yuv420p"),
    "tinted_lit_instances_between_instanced_test_write": _tinted_lit_between_instanced(True, True),
    "tinted_lit_instances_between_instanced_test_only": _tinted_lit_between_instanced(True, False),
    "tinted_lit_instances_between_instanced_depth_off": _tinted_lit_between_instanced(False, False),
    # a textured buffer drawn warm under another filter than the draw that left its tile lists
    "warm_textured_buffer_across_filter_changes": (
        _knobs(warm=1), dict(texs=[RGB_TEX], bufs=[("t", 120, 32, 40.0, "const")], meshes=[]),
        [("buf", 0, ("res", 0)), ("filter", 1), ("buf", 0, ("res", 0)), ("cleardepth", 0xFFFFFFFF), ("filter", 0),
         ("buf", 0, ("res", 0)), ("filter", 1), ("buf", 0, ("res", 0))]),
    "lit_mesh_updated_while_its_draw_is_pending": (
        _knobs(paircap=50), dict(texs=[], bufs=[], meshes=[LIT_MESH]),
        [("lights", 4, 3), ("lmesh2", 0, 1, 12, 13), ("readdepth",)]),
    # ---- the wrap state, modulated, posed and morphed draws (tests/frame_anim.py) ----
    # a textured buffer drawn warm under another wrap than the draw that left its tile lists
    "warm_textured_buffer_across_wrap_changes": (
        _knobs(warm=1), dict(texs=[RGB_TEX], bufs=[("t", 120, 32, 40.0, "tiled")], meshes=[]),
        [("buf", 0, ("res", 0)), ("wrap", 1, 2), ("buf", 0, ("res", 0)), ("cleardepth", 0xFFFFFFFF), ("wrap", 0, 0),
         ("buf", 0, ("res", 0)), ("wrap", 2, 1), ("buf", 0, ("res", 0))]),
    "recorded_wrap_and_filter_flushed_once": (
        _knobs(record=True), dict(texs=[RGB_TEX], bufs=[("t", 120, 32, 40.0, "tiled")], meshes=[TC_MESH]),
        [("buf", 0, ("res", 0)), ("wrap", 1, 1), ("filter", 1), _MOD, ("wrap", 2, 0), ("filter", 0),
         ("ttri", "host", 100, 33, 40.0, "tiled", ("res", 0)), ("wrap", 0, 1), ("mesh", 0, 0, ("res", 0))]),
    # the pose kernels between draws whose batches overflow and are re-run later: each re-run reads its own staging
    "pose_and_morph_between_pending_draws_over_cap": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[], meshes=[LIT_MESH], rigs=[RIG], morphs=[MORPH]),
        [("lights", 4, 3), ("mesh", 0, 0, ("res", 0)), ("pose", 0, 7, "host", "main"), ("mesh", 0, 1, ("res", 0)),
         ("morph", 0, 8, 3, "dev", "main"), ("lmesh", 0, 0, 12), ("posemorph", 0, 9, 10, None, "host", "main"),
         ("meshi", 0, 3, 31, "opaque", "host"), ("readdepth",)]),
    "posed_mesh_as_every_draw_kind_in_one_depth_buffer_test_write": _posed_as_every_draw_kind(True, True),
    "posed_mesh_as_every_draw_kind_in_one_depth_buffer_test_only": _posed_as_every_draw_kind(True, False),
    "posed_mesh_as_every_draw_kind_in_one_depth_buffer_depth_off": _posed_as_every_draw_kind(False, False),
    "pose_issued_on_the_auxiliary_context": (
        _knobs(), dict(texs=[RGB_TEX], bufs=[], meshes=[LIT_MESH], rigs=[RIG], morphs=[MORPH]),
        [("lights", 4, 3), ("lmesh", 0, 1, 12), ("pose", 0, 7, "dev", "aux"), ("lmesh", 0, 1, 12),
         ("morph", 0, 9, None, "host", "aux"), ("mesh", 0, 1, ("res", 0)), ("readf64",)]),
    "modulated_kinds_in_one_depth_buffer": (
        _knobs(), dict(texs=[RGB_TEX], bufs=[], meshes=[TL_MESH]),
        [("lights", 4, 3), ("wrap", 2, 1), ("tri", "host", 150, 11, 40.0, False, False), _MOD, _MOD_BLENDED,
         ("lmesh", 0, 1, 12)]),
    "wrapped_shared_snapshot_survives_the_rerun": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[], meshes=[]),
        [("grd", [0.9, 0.1, 0.4, 1.0], [0.0, 0.0, 200.0, 140.0]), ("tri", "host", 40, 51, 40.0, True, False), ("wrap", 1, 1),
         ("mtri", "host", 300, 52, 40.0, "flat", False, None, ("snap", "main", True)), ("wrap", 2, 2),
         ("ttri", "host", 300, 53, 40.0, "tiled", ("snap", "main", True)), ("begin",),
         ("tex", ("snap", "main", True), [20.0, 10.0, 90.0, 60.0]), ("end",)]),
    # the lit entry above with a lit textured colour mesh first: its staged uv and colours beside the soup
    "lit_textured_rerun_after_the_staging_regrows_and_shrinks": (
        _knobs(paircap=50), dict(texs=[RGB_TEX], bufs=[], meshes=[TL_MESH, ("c", "model", 10, 10, 4, True, False), TU_MESH]),
        [("lights", 4, 3), ("wrap", 1, 2), ("lmesh", 0, 1, 12), ("lights", 5, 8), ("near", 0.5), ("cull", 1),
         ("meshi", 0, 5, 31, "opaque", "host"), ("mesh", 2, 2, ("res", 0))]),
    "six_states_survive_save_resize_restore_clear": _six_states_survive("yuv420p"),
}


def _expect(name, frame, got):
    """The sequence took the road it is named after."""
    paths = [p for _, p, _ in got["batches"]]
    pairs = [n for _, _, n in got["batches"]]
    if name.startswith("six_buffer"):
        assert paths == ["order-free"] * 6 and min(pairs) > 50
    if name.startswith("overflowing") or name.startswith("shared_frame") or name.startswith("rerun_keeps"):
        assert max(pairs) > 50 and "order-free" in paths
    if name.startswith("kinds_in_one"):
        assert paths == ["order-free", "order-free", "ordered", "ordered", "order-free"]
    if name.startswith("moved_mesh"):
        assert got["warm"] > 0 and len(paths) == 6
    if name.startswith("fast_clear"):
        assert paths == ["order-free"] * 2      # and both batches stay inside the top-left tiles
        assert (got["depth"][40:] == 0xFFFFFFF0).all() and (got["depth"][:, 140:] == 0xFFFFFFF0).all()
        assert (got["depth"][:32, :64] != 0xFFFFFFF0).any()
    if name.startswith("texture_shared"):
        assert paths == ["order-free"] if not frame[2] else paths == ["ordered"]
    kinds, counts = [k for k, _, _ in got["batches"]], got["counts"]
    if name.startswith("lit_rerun"):
        assert kinds == ["lit", "instanced", "mesh"] and pairs[0] > 50 and got["changed_over_cap"] == 3
        assert counts[0] == (192, 192) and counts[1][0] == 1000 and counts[2][0] == 40      # regrown, then smaller
        assert 0 < counts[1][1] != 1000 and 0 < counts[2][1] != 40                          # both under the clip stage
    if name.startswith("recorded_filter"):
        assert frame[3]["record"] and not any(op[0] in ("flush", "end") for op in frame[5])
        assert kinds == ["textured", "mesh", "textured"] and counts == [(40, 40)]
    if name.startswith("states_survive"):
        assert kinds == ["instanced", "lit", "lit", "lit", "lit", "textured"]
        assert got["f64"].shape[:2] == (100, 150) and frame[3]["coop"] == 2 and "frame" in got
        assert all(0 < n < full for full, n in counts)         # near plane and cull mode reached every mesh draw
    if name.startswith("tinted_lit"):
        assert kinds == ["instanced", "lit", "instanced"] and paths == ["order-free", "ordered", "order-free"]
    if name.startswith("warm_textured"):
        assert kinds == ["textured"] * 4 and got["warm"] >= 2
    if name.startswith("lit_mesh_updated"):
        assert kinds == ["lit", "lit"] and min(pairs) > 50
    if name.startswith("warm_textured_buffer_across_wrap"):
        assert kinds == ["textured"] * 4 and got["warm"] >= 2
    if name.startswith("recorded_wrap"):
        assert frame[3]["record"] and not any(op[0] in ("flush", "end") for op in frame[5])
        assert kinds == ["textured", "modulated", "textured", "modulated"] and counts == [(60, 60)]
    if name.startswith("pose_and_morph"):
        assert kinds == ["mesh", "mesh", "lit", "instanced"] and min(pairs) > 50
        assert got["posed_between"] == 3 and got["posed_over_cap"] == 3 and got["posed"] == 1
    if name.startswith("posed_mesh_as_every"):
        assert kinds == ["colour", "mesh", "instanced", "modulated", "lit", "lit"] and got["posed"] == 1
        assert all(0 < n < full for full, n in counts)         # near plane and cull mode reached every draw of the posed mesh
    if name.startswith("pose_issued"):
        assert kinds == ["lit", "lit", "mesh"] and got["posed_between"] == 2 and got["posed"] == 1
    if name.startswith("modulated_kinds"):
        assert kinds == ["colour", "modulated", "modulated", "modulated"]
        assert paths == ["order-free", "order-free", "ordered", "order-free"]
    if name.startswith("wrapped_shared"):
        assert kinds == ["colour", "modulated", "textured"] and min(pairs[1:]) > 50 and "order-free" in paths
        assert got["wrap_over_cap"] == 2            # (behind the colour batch, then behind the modulated one)
    if name.startswith("lit_textured_rerun"):
        assert kinds == ["modulated", "instanced", "mesh"] and pairs[0] > 50 and got["changed_over_cap"] == 3
        assert counts[0] == (150, 150) and counts[1][0] == 1000 and counts[2][0] == 40      # regrown, then smaller
        assert 0 < counts[1][1] != 1000 and 0 < counts[2][1] != 40                          # both under the clip stage
    if name.startswith("six_states"):
        assert kinds == ["instanced", "lit", "modulated", "textured", "modulated"]
        assert got["f64"].shape[:2] == (100, 150) and frame[3]["coop"] == 2 and "frame" in got
        assert all(0 < n < full for full, n in counts)         # near plane and cull mode reached every mesh draw


@pytest.mark.parametrize("alpha", [False, True], ids=["rgb", "rgba"])
@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_sequence(gpu, oracle, name, alpha):
    knobs, res, ops = FIXED[name]
    frame = (W, H, alpha, knobs, res, ops)
    _expect(name, frame, _compare(gpu, oracle, frame, run=A.run))
