"""Which passes a mesh draw runs (the mesh front end): every kind
of draw, with kernel timing on for exactly that draw, reports one launch under
each timing id of its passes and none under any other mesh id, and its frame is
the reference frame the sibling test files derive for it.  Then all the draws
back to back on one context, large and small meshes in turn: each draw's
Assemble* soup against its reference -- the staging is carved afresh for every
layout after a different one has used it."""
import collections
import functools

import numpy as np
import pytest

import mesh_clip_ref as MC
import mesh_inst_ref as MI
import mesh_light_ref as ML
import mesh_ref as MR
import mesh_skin_ref as MS
import modulate_ref as M
import persp_ref as P
import scenes

pytestmark = pytest.mark.gpu

W, H = MI.W, MI.H
CT = (0.9, 0.8, 0.7, 1.0)
FAR = 0xFFFFFFFF
A, LIGHTS = ML.AMBIENT, ML.LIGHTS
ROT = ML.rotation3()
K = 3

SINGLE = ("vertex", "assemble", "clip_vertex", "clip_count", "clip_scan", "clip_emit", "light", "lit_attr")
NAMES = tuple("mesh_" + p for p in SINGLE) + tuple("mesh_inst_" + p for p in SINGLE) + ("mesh_skin",)
assert len(NAMES) == 17

CLIP = ("clip_vertex", "clip_count", "clip_scan", "clip_emit")
CLIP_LIT = ("clip_vertex", "clip_count", "clip_scan", "light", "lit_attr", "clip_emit")

# kind: a colour mesh or a textured colour mesh; near: the near plane (0: the clip state off)
Row = collections.namedtuple("Row", "name kind passes near cull persp lit inst")
ROWS = (
    Row("draw_mesh", "colour", ("vertex", "assemble"), 0.0, 0, False, False, False),
    Row("draw_mesh, near plane", "colour", CLIP, MI.NEAR, 0, False, False, False),
    Row("draw_mesh_lit", "colour", ("vertex", "light", "assemble"), 0.0, 0, False, True, False),
    Row("draw_mesh_lit, near plane", "colour", CLIP_LIT, MI.NEAR, 0, False, True, False),
    Row("draw_mesh_lit, everything behind the plane", "colour", CLIP[:3], 1e6, 0, False, True, False),
    Row("textured colour, unlit", "texc", ("vertex", "assemble"), 0.0, 0, False, False, False),
    Row("textured colour, unlit, perspective", "texc", ("vertex", "assemble"), 0.0, 0, True, False, False),
    Row("textured colour, lit", "texc", ("vertex", "light", "assemble"), 0.0, 0, False, True, False),
    Row("textured colour, lit, near plane", "texc", CLIP_LIT, P.NEAR, 0, False, True, False),
    Row("instanced", "colour", ("vertex", "assemble"), 0.0, 0, False, False, True),
    Row("instanced, near plane", "colour", CLIP, MI.NEAR, 1, False, False, True),
    Row("lit instanced, tint", "colour", ("vertex", "light", "assemble"), 0.0, 0, False, True, True),
    Row("lit instanced, tint, near plane", "colour", CLIP_LIT, MI.NEAR, 1, False, True, True),
)


def _R():
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    return R


@functools.lru_cache(maxsize=None)
def _mesh(kind, small):
    """The 320-triangle spheres of the sibling files, or a 2-triangle mesh of 4 vertices."""
    if small:
        mesh = M.random_textured_color_mesh(4, 2, seed=9)
        return mesh if kind == "texc" else {k: v for k, v in mesh.items() if k != "uv"}
    return M.lit_textured_sphere(rows=10, cols=16) if kind == "texc" else ML.lit_sphere3d()


def _gpu_mesh(mesh):
    return _R().Mesh(mesh["pos"], mesh["idx"], colors=mesh["colors"], uv=mesh.get("uv"), gouraud=True,
                     normals=mesh["normals"])


@functools.lru_cache(maxsize=None)
def _instances():
    """Three of the instanced scene's placements (a random one, the eye inside the sphere, another random one),
    their normal matrices and tints."""
    mats = np.ascontiguousarray(MI.scene_matrices()[[0, MI.BEHIND, 1]])
    g = scenes.rng(21)
    normals = np.stack([ML.rotation3(g.uniform(-3, 3), g.uniform(-3, 3)) for _ in range(K)])
    return mats, normals, MI.scene_tints(K)


def _matrix(row):
    return MR.behind_eye(W, H) if row.near else MR.perspective(W, H)


def _clear(row):
    return FAR if row.near else MR.CLEAR


def _state(ctx, row):
    """A cleared frame under the row's state."""
    MR.begin_frame(ctx, "zw", MR.XFORM, CT, clear=_clear(row))
    ctx.set_mesh_near_plane(row.near)
    ctx.set_mesh_cull(row.cull)
    ctx.set_mesh_perspective(row.persp)
    ctx.set_triangle_texture_filter(0)
    ctx.set_mesh_lights(A, LIGHTS)


def _draw(ctx, row, gm, tex):
    mats, normals, tint = _instances()
    if row.inst and row.lit:
        ctx.draw_mesh_lit_instanced(gm, mats, normals, tint)
    elif row.inst:
        ctx.draw_mesh_instanced(gm, mats)
    elif row.lit:
        ctx.draw_mesh_lit(gm, _matrix(row), ROT, texture=tex if row.kind == "texc" else None)
    else:
        ctx.draw_mesh(gm, _matrix(row), texture=tex if row.kind == "texc" else None)


def _assemble(ctx, row, gm):
    mats, normals, tint = _instances()
    if row.kind == "texc":
        return ctx.assemble_textured_color_mesh(gm, _matrix(row), ROT, lit=row.lit)
    if row.inst and row.lit:
        return ctx.assemble_mesh_lit_instanced(gm, mats, normals, tint)
    if row.inst:
        return ctx.assemble_mesh_instanced(gm, mats)
    if row.lit:
        return ctx.assemble_mesh_lit(gm, _matrix(row), ROT)
    return ctx.assemble_mesh_clipped(gm, _matrix(row))


def _want_soup(row, mesh):
    mats, normals, tint = _instances()
    if row.kind == "texc":
        return M.mesh_soup(mesh, _matrix(row), row.lit, ROT, A, LIGHTS, row.near, row.cull, row.persp)
    if row.inst and row.lit:
        return ML.lit_instanced_soup(mesh, mats, normals, tint, A, LIGHTS, row.near, row.cull)
    if row.inst:
        return MI.instanced_soup(mesh, mats, None, row.near, row.cull)
    if row.lit:
        return ML.lit_soup(mesh, _matrix(row), ROT, A, LIGHTS, row.near, row.cull)
    clip = row.near > 0 or row.cull != 0
    return MC.clip_soup(mesh, _matrix(row), row.near, row.cull)[:3] if clip else MR.expand(mesh, _matrix(row))


@functools.lru_cache(maxsize=None)
def _want_frame(row):
    """The reference frame of the row's draw of the large mesh, derived as its own test file derives it."""
    mesh = _mesh(row.kind, False)
    if row.kind == "texc":
        b = M.mesh_batch(mesh, _matrix(row), P.mesh_texture(False), ct=CT, lit=row.lit, N=ROT, ambient=A, lights=LIGHTS,
                         w_near=row.near, cull=row.cull, persp=row.persp)
        return M.expected_payload(W, H, False, MR.BG, "zw", _clear(row), [b], filt=0)
    mats, normals, tint = _instances()
    if row.inst:
        draws = ML.instance_meshes(mesh, mats, normals, tint, A, LIGHTS) if row.lit else MI.instance_meshes(mesh, mats)
    else:
        draws = [(ML.lit_mesh(mesh, ROT, A, LIGHTS) if row.lit else mesh, _matrix(row))]
    return ML.oracle_frame(W, H, False, "zw", draws, row.near, row.cull, ct=CT, clear=_clear(row))


def _soup_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, k)
        if w is not None:
            assert MS.same_bits(g, w), (what, k, g.shape, w.shape, scenes.first_mismatch(g, w))


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_a_draw_reports_its_passes_and_no_others(gpu, row):
    mesh = _mesh(row.kind, False)
    gm = _gpu_mesh(mesh)
    tex = gpu.texture(P.mesh_texture(False))
    ctx = gpu.context(W, H, False)
    _state(ctx, row)
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    ctx.enable_kernel_timing(True)
    _draw(ctx, row, gm, tex)
    ctx.enable_kernel_timing(False)
    got = {name: ctx.get_kernel_timing(name)[1] for name in NAMES}
    prefix = "mesh_inst_" if row.inst else "mesh_"
    want = {name: int(name in {prefix + p for p in row.passes}) for name in NAMES}
    print(row.name, {k: v for k, v in got.items() if v})
    assert got == want, (row.name, {k: (got[k], want[k]) for k in NAMES if got[k] != want[k]})
    assert ctx.mesh_last_triangle_count == _want_soup(row, mesh)[0].shape[0]
    frame, wanted = MR.read_frame(ctx, "zw"), _want_frame(row)
    assert scenes.bits_equal(frame[0], wanted[0]), (row.name, scenes.first_mismatch(frame[0], wanted[0]))
    assert np.array_equal(frame[1], wanted[1]), (row.name, "depth", scenes.first_mismatch(frame[1], wanted[1]))


def test_every_layout_after_every_other_on_one_context(gpu):
    tex = gpu.texture(P.mesh_texture(False))
    gms = {(kind, small): _gpu_mesh(_mesh(kind, small)) for kind in ("colour", "texc") for small in (False, True)}
    ctx = gpu.context(W, H, False)
    for parity in (0, 1):                                     # each draw with the large and with the small mesh
        for i, row in enumerate(ROWS):
            small = (i + parity) % 2 == 1
            _state(ctx, row)
            _draw(ctx, row, gms[row.kind, small], tex)
            want = _want_soup(row, _mesh(row.kind, small))
            assert ctx.mesh_last_triangle_count == want[0].shape[0], (row.name, small)
            _soup_same(_assemble(ctx, row, gms[row.kind, small]), want, (row.name, "small" if small else "large"))
