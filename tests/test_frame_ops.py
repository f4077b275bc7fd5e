"""The frame vocabulary on the oracle alone (no GPU): its lowerings are what
tests/frame_ops.py claims, and the frames its strategies generate -- exactly
the examples tests/test_fuzz_mixed_gpu.py runs -- are worth running."""
import numpy as np
import pytest

import frame_ops as F
import mesh_ref as MR
import scenes
import textured_ref as T


def test_flat_colours_on_a_2x2_texture_is_texel_zero():
    g = scenes.rng(11)
    for ch in (3, 4):
        tex = g.uniform(0, 1, size=(2, 2, ch))
        uv = np.concatenate([g.uniform(-1e6, 1e6, size=(500, 2)), g.uniform(-3, 5, size=(500, 2)),
                             [[0.0, 0.0], [1.0, 1.0], [-0.0, 2.0], [1e300, -1e300], [0.999, 1.001]]])
        want = np.concatenate([tex[0, 0], [1.0]])[:4] if ch == 3 else tex[0, 0]
        got = T.flat_colours(tex, uv)
        assert got.shape == (uv.shape[0], 4)
        assert scenes.bits_equal(got, np.ascontiguousarray(np.broadcast_to(want, got.shape)))


@pytest.mark.parametrize("space", ["screen", "model"])
def test_unshared_mesh_expands_to_its_soup(space):
    spec = ("tu", space, 57, 1234, 0.3)
    mesh = F.mesh_dict(spec, 140, 110)
    xy, z, uv = F.mesh_soup(spec, 140, 110)
    assert sorted(mesh["idx"].reshape(-1).tolist()) == list(range(3 * 57))      # a permutation: no vertex shared
    assert not np.array_equal(mesh["idx"].reshape(-1), np.arange(3 * 57))
    for M in (None, MR.IDENT16):
        gxy, gz, guv = MR.expand(mesh, M)
        assert scenes.bits_equal(gxy, xy) and scenes.bits_equal(gz, z) and scenes.bits_equal(guv, uv)
    assert np.array_equal(uv[:, 0:2], uv[:, 2:4]) and np.array_equal(uv[:, 0:2], uv[:, 4:6])   # one UV per triangle


FIXED = (97, 61, True, F.KNOBS_OFF,
         dict(texs=[(9, 7, 4, "u8", 5, None), (20, 11, 3, "f64", 6, (5, 4))],
              bufs=[("c", 40, 1, 40.0, True, False), ("t", 30, 2, 40.0, "const")],
              meshes=[("c", "model", 4, 6, 3, True, False), ("tu", "screen", 20, 4, 0.3)]),
         [("tri", "dev8", 50, 7, 40.0, False, True), ("buf2", 1, ("res", 0), 1.5), ("mesh2", 0, 2, ("res", 0), 9),
          ("tex", ("snap", "main", True), [3.0, 4.0, 50.0, 30.0]), ("aux", "tri", [0.2, 0.3, 0.4, 0.3], [1.0, 2.0, 3.0, 4.0]),
          ("ttri", "host", 30, 8, 40.0, "const", ("snap", "aux", True)), ("getcolor", 30.0, 20.0), ("readdepth",),
          ("mesh", 1, 1, ("res", 1)), ("ttri", "dev", 20, 9, 6.0, "free", ("tiny", 3, 4)), ("gather",),
          ("resize", 50, 40), ("buf", 0, ("tiny", 1, 3)), ("stex", ("res", 1), [1.0, 2.0, 30.0, 30.0], [0.1, 0.9, 0.2, 0.8])])


def test_run_on_the_oracle_is_deterministic(oracle):
    a, b = F.run(oracle, FIXED), F.run(oracle, FIXED)
    assert F.mismatches(a, b) == [] and len(a["probes"]) == 2
    assert a["batches"] == b["batches"] and len(a["batches"]) == 10
    assert a["f64"].shape == (40, 50, 4)
    bare = F.run(oracle, FIXED, triangles=False)
    assert bare["batches"] == [] and not scenes.bits_equal(bare["f64"], a["f64"])
    assert F.kinds(FIXED) <= set(F.ALL_KINDS)


def _fraction(flags):
    return sum(bool(f) for f in flags) / max(len(flags), 1)


@pytest.mark.parametrize("size", ["small", "large"])
def test_generated_frames_are_worth_running(oracle, size):
    """The examples of the GPU property tests (the same strategies, settings
    and derandomize=True, frame_ops.for_each_frame), on the oracle only."""
    frames, changed, finite = [], [], []

    def visit(fr):
        frames.append(fr)
        out = F.run(oracle, fr)
        finite.append(all(np.isfinite(a).all() for a in [out["f64"]] + [p for p in out["probes"] if p.dtype == np.float64]))
        if out["batches"]:
            bare = F.run(oracle, fr, triangles=False)
            changed.append(not scenes.bits_equal(out["f64"], bare["f64"]))

    F.for_each_frame(size, visit)
    assert len(frames) >= {"small": 150, "large": 20}[size]
    assert all(finite), "an oracle frame holds a NaN or an infinity"
    report = {}
    if size == "small":
        used = [F.kinds(fr) for fr in frames]
        assert set().union(*used) <= set(F.ALL_KINDS)
        for k in F.ALL_KINDS:
            report[k] = _fraction([k in u for u in used])
        low = {k: v for k, v in report.items() if v < 0.10}
        assert not low, f"operation kinds in fewer than 10 % of the frames: {low}"
        for knob, values in F.KNOB_VALUES.items():
            for v in values:
                f = _fraction([fr[3][knob] == v for fr in frames])
                assert f >= 0.15, f"knob {knob}={v!r} in {f:.0%} of the frames"
        mixed = _fraction([any(len(e) >= 2 for e in F.batch_kinds(fr)[0]) for fr in frames])
        assert mixed >= 0.30, f"{mixed:.0%} of the frames mix triangle kinds in one depth buffer"
        four = _fraction([F.batch_kinds(fr)[1] >= 4 for fr in frames])
        assert four >= 0.25, f"{four:.0%} of the frames hold four or more triangle batches"
    assert len(changed) >= len(frames) // 2
    assert _fraction(changed) >= 0.80, f"the triangles change {_fraction(changed):.0%} of the frames that hold some"
