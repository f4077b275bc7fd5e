"""CPU checks of the primitive edge fuzz (tests/prim_fuzz.py): the generators
are deterministic, every case runs on the oracle with finite outputs that match
the committed digests, and the cases reach what they claim -- decided by the
Python restatements of the host-side decisions in prim_fuzz.py, never by the
library.  The DrawLine cull (the one place where the library scans fewer
pixels than the reference) is pinned here against the oracle's full scan."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import prim_fuzz as P

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = list(P.FAMILIES)


@functools.lru_cache(maxsize=None)
def _traces(family):
    """(case, oracle outputs, per-draw records) of every case of the family,
    computed once and shared by the tests below."""
    import scenes
    fac = scenes.OracleFactory()
    return [(c,) + P.trace(c, fac) for c in P.cases(family)]


def _draw_arms(family):
    """(case, record, queued ranges, arms) of every draw of the family."""
    for case, _, recs in _traces(family):
        W, H, _ = case["ctx"]
        for r in recs:
            ranges, arms = P.py_ranges(r["op"], r["m"], W, H)
            yield case, r, ranges, arms


# ---- determinism ---------------------------------------------------------------
def test_cases_are_the_same_in_a_fresh_interpreter():
    here = {c["name"]: P.digest(c) for c in P.all_cases()}
    code = ("import sys, json; sys.path.insert(0, %r); import prim_fuzz as P; "
            "print(json.dumps({c['name']: P.digest(c) for c in P.all_cases()}))" % HERE)
    env = dict(os.environ, PYTHONHASHSEED="random")
    there = json.loads(subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True,
                                      env=env).stdout)
    assert here == there
    assert len(here) == sum(n for _, n in P.FAMILIES.values())


def test_case_shapes_stay_inside_the_stated_sets():
    for c in P.all_cases():
        W, H, _ = c["ctx"]
        assert W in P.WIDTHS and H in P.HEIGHTS, c["name"]
        for w, h, dtype, ch, _ in c["textures"]:
            assert (w, h) in P.TEX_SHAPES and dtype in ("u8", "f64") and ch in (3, 4), c["name"]
    alphas = {(f, c["ctx"][2]) for f in FAMILIES for c in P.cases(f)}
    assert alphas == {(f, a) for f in FAMILIES for a in (False, True)}     # every family on RGB and on RGBA
    pix = {c["ctx"] for c in P.cases("pixels")}
    assert pix == {(W, H, a) for W in P.WIDTHS for H in P.HEIGHTS for a in (False, True)}


# ---- oracle outputs ------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_outputs_are_finite_and_match_the_committed_digests(family):
    with open(os.path.join(HERE, "golden", "prim_fuzz.sha256")) as f:
        golden = dict(line.split() for line in f if line.strip())
    for case, out, _ in _traces(family):
        assert np.isfinite(out["f64"]).all() and np.isfinite(out["probes"]).all(), case["name"]
        assert all(np.isfinite(m).all() for m in out["made"]), case["name"]
        assert all(isinstance(b, bool) for b in out["bools"]), case["name"]
        for line in P.golden_lines(case, out):
            key, sha = line.split()
            assert golden.get(key) == sha, key
    mine = {k for k in golden if k.split("-")[0] == family}
    want = {line.split()[0] for case, out, _ in _traces(family) for line in P.golden_lines(case, out)}
    assert mine == want                                                    # no stale entry


# ---- the cases reach what they claim -------------------------------------------
@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "pixels"])
def test_draws_draw(family):
    """Every draw that is not marked empty changes a pixel when run alone on the
    oracle (at most one in ten across the family may not), and a draw marked
    empty changes none."""
    n = blank = 0
    for case, _, recs in _traces(family):
        for r in recs:
            if r["i"] in case["empty"]:
                assert not r["mask"].any(), (case["name"], r["i"], r["op"])
            else:
                n += 1
                blank += not r["mask"].any()
        assert set(case["empty"]) <= {r["i"] for r in recs}, case["name"]
    assert n > 0 and blank * 10 <= n, (family, blank, n)


def test_fastpath_reaches_both_sides_of_the_threshold():
    near = {True: 0, False: 0}
    sides = set()
    for case, r, _, arms in _draw_arms("fastpath"):
        if r["op"][0] != "draw_texture":
            continue
        m = r["m"]
        s = m[0] - 1 + m[1] + m[2] + m[3] - 1 + m[4] + m[5]
        assert ("fast" in arms) == (s < 1e-5) == P.py_is_no_transform(m)
        if abs(s - 1e-5) <= 1.0000001e-6:
            near[s < 1e-5] += 1
        if s < -100:
            sides.add("large negative translation")
        if m[4] == 0 and m[5] == 0 and m[0] == m[3] and m[1] == -m[2] and m[1] != 0:
            sides.add("pure rotation on the fast path" if "fast" in arms else "pure rotation, inverse")
    assert near[True] >= 3 and near[False] >= 3, near
    assert {"large negative translation", "pure rotation on the fast path"} <= sides, sides


def test_line_reaches_the_cull_and_both_fallbacks():
    kinds = {}
    for case, r, _, arms in _draw_arms("line"):
        for a in arms:
            if a.startswith("line_") and r["mask"].any():
                kinds[a] = kinds.get(a, 0) + 1
    assert set(kinds) == {"line_cull", "line_singular", "line_nonfinite"}, kinds


def test_bounds_reaches_the_saturating_arms():
    seen = set()
    for case, r, _, arms in _draw_arms("bounds"):
        seen |= arms
        if r["mask"].any():
            seen |= {a + ":drawn" for a in arms}
    assert {"long_max:drawn", "long_min:drawn", "f2i64_long_min:drawn", "f2i64_long_min"} <= seen, seen
    # fast_range's two ceil correction loops cannot run: they are entered only below 9.0e15 < 2^53,
    # where ceil(lim), ceil(lim) - 1 and their doubles are exact
    assert not {"ceil_down", "ceil_up"} & seen


def test_transform_reaches_every_determinant_class():
    dets = [r["m"][0] * r["m"][3] - r["m"][1] * r["m"][2] for _, _, recs in _traces("transform") for r in recs]
    assert any(d == 0 for d in dets) and any(d < 0 for d in dets)
    assert any(0 < d < 2.3e-308 for d in dets)                             # subnormal
    assert any(0 < abs(d) < 1e-11 and abs(d) > 1e-300 for d in dets)       # near zero, normal
    for case, out, _ in _traces("transform"):
        assert out["bools"][0] is False and out["bools"][-1] is False and True in out["bools"], case["name"]


def test_list_cases_hit_their_tile_the_intended_number_of_times():
    """The per-tile hit counts, recomputed from the queued pixel ranges, are the
    intended K, and each list_len operation names the number of commands queued
    since the queue last ran or was dropped (checked on the GPU)."""
    seen_k = set()
    for case, _, _ in _traces("list"):
        W, H, _ = case["ctx"]
        ranges = []
        m = P.IDENT
        for op in case["ops"]:
            assert op[0] not in P.STATE_OPS, "the list cases draw under the identity"
            if op[0] in P.QUEUED_OPS:
                rs, _ = P.py_ranges(op, m, W, H)
                aux_tex = case["aux"] is not None and op[0] in ("draw_texture", "draw_split") and \
                    op[1] == len(case["textures"])
                if aux_tex:
                    ranges = []            # a shared texture: the queue runs, then the draw, at once
                else:
                    ranges += rs
            elif op[0] in ("get_color", "snapshot") or (op[0] == "set_color"):
                ranges = []
            elif op[0] == "list_len":
                assert op[1] == len(ranges), (case["name"], op, len(ranges))
                if "tile" in case and op is case["ops"][-1]:
                    tx, ty = case["tile"]
                    assert tx * P.CL_W < W and ty * P.CL_H < H
                    assert sum(P.hits_tile(r, tx, ty) for r in ranges) == case["K"], case["name"]
                    if case["K"] == 1:     # no hit in the first round of 256, one in the second
                        assert not any(P.hits_tile(r, tx, ty) for r in ranges[:256])
                        assert P.hits_tile(ranges[256], tx, ty)
                    seen_k.add(case["K"])
        assert case["ops"][-1][0] == "list_len", case["name"]
    assert {255, 256, 257, 512, 513, 1, 0} <= seen_k
    assert {c["ctx"][0] for c in P.cases("list")} >= {2, 64, 65, 129}


def test_texel_and_resample_cover_every_texture_kind():
    for fam in ("texel", "resample"):
        kinds = {(w, h, d, ch) for c in P.cases(fam) for w, h, d, ch, _ in c["textures"]}
        assert kinds == {(w, h, d, ch) for w, h in P.TEX_SHAPES for d in ("u8", "f64") for ch in (3, 4)}, fam
    for c in P.cases("resample"):
        made = [(op[2], op[3]) for op in c["ops"] if op[0] == "resample"]
        assert {(1, 1), (3, 7), (7, 3)} <= set(made)
        assert all((2 * w, 2 * h) in made for w, h in P.TEX_SHAPES)
    # the 49 -> 49 resample is there because the rounding of (f64)x / W * tw decides a texel in it ...
    assert any(int(x / 49 * 49) != x for x in range(48))
    for case, out, _ in _traces("resample"):
        src, dst = out["made"][-4], out["made"][-3]                       # 49x3 and its 49x3 resample
        assert src.shape == dst.shape == (3, 49, src.shape[2])
        assert int(16 / 49 * 49) == 15                                    # (columns 15 and 16 hold different source texels)
        assert np.array_equal(dst[0, 16], src[0, 15]) and not np.array_equal(dst[0, 16], src[0, 16])
    # ... and in no other: with sources up to 16 texels and targets below 400 it truncates like the exact quotient
    for t in (1, 2, 3, 5, 9, 12, 16):
        for W in range(1, 400):
            assert all(int(x / W * t) == x * t // W for x in range(W)), (t, W)


def test_blend_products_are_what_they_claim():
    prods = set()
    for c in P.cases("blend"):
        ct3 = 1.0
        for op in c["ops"]:
            if op[0] == "set_ct":
                ct3 = op[4]
            elif op[0] in ("draw_rect", "draw_circle", "draw_line"):
                a = op[-1] * ct3
                prods.add("one" if a == 1 and op[-1] != 1 else "up" if a == P.up(1.0) else
                          "down" if a == P.down(1.0) else "zero" if a == 0 else "neg" if a < 0 else
                          "above" if a > 1 else "other")
    assert {"one", "up", "down", "zero", "neg", "above"} <= prods, prods


# ---- the DrawLine cull ---------------------------------------------------------
def test_line_cull_box_holds_every_pixel_of_the_full_scan():
    """The oracle scans the whole frame for a line, as the reference does
    (cpp:876-918); the library scans the box of nr_prims.hip DrawLine.  No pixel
    the full scan covers may lie outside that box."""
    lines = culled = 0
    for family in ("line", "transform"):
        for case, r, ranges, arms in _draw_arms(family):
            if r["op"][0] != "draw_line":
                continue
            lines += 1
            ys, xs = np.nonzero(r["mask"])
            if len(xs) == 0:
                continue
            assert ranges, (case["name"], r["i"], "covered pixels, but the host queues nothing")
            i0, i1, j0, j1 = ranges[0]
            assert xs.min() >= i0 and xs.max() < i1 and ys.min() >= j0 and ys.max() < j1, \
                (case["name"], r["i"], r["op"], r["m"], ranges[0])
            W, H, _ = case["ctx"]
            culled += "line_cull" in arms and (i1 - i0) * (j1 - j0) < W * H
    assert lines >= 300 and culled >= 50, (lines, culled)
