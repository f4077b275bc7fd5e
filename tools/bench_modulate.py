"""What a lit, textured mesh draw costs: tools/bench_filter.py's scene (the
turning C3 sphere: 501 x 1001 vertices, 1M triangles, depth write, 3840x2160, a
1024x1024 RGB texture, a new perspective matrix every frame) drawn four ways --
the same frames, in one process on one GPU, in alternating groups (a1, a2, b,
c, a1, a2, b, c, ...):

  a1  DrawTexturedMeshLit of the textured colour mesh, SetMeshPerspective off
      (q == 1: the modulated mode's divide is paid for an affine map)
  a2  the same with SetMeshPerspective on
  b   DrawTexturedMesh of the plain textured mesh, SetMeshPerspective on
  c   DrawMeshLit of the lit colour mesh, the same geometry, matrices and lights

a is one binning and one raster; b + c is what a caller pays without the
modulated mode for two draws that still do not give this picture.  Wall-clock ms
per frame (host clock around frames that end in a flush) after a clock settle
and warmup, the median of the groups and their spread; then the library's
kernel timing (GetKernelTiming) of the raster in each configuration.  Reported:
a / b for frame and raster kernel with the spread over the groups, and the bar
a < b + c on the medians.

The last timed frame of a 1/16-size version (960x540, a 125 x 250 mesh) of a2 is
verified against tests/modulate_ref.py's expected frame.

    python tools/bench_modulate.py --steps 40 --warmup 5 --out profiles/modulate/ab_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_mesh_lit as BL   # noqa: E402  (the lit model, the normal matrices, the lights)
import bench_persp as BP      # noqa: E402  (the texture coordinates, the perspective matrices)

KERNELS = ("tile_raster",)


def model(BM, H, rows, cols):
    """bench_mesh_lit's lit sphere with bench_persp's texture coordinates."""
    mesh, radius = BL.lit_model(H, rows, cols)
    mesh["uv"] = BP.textured_model(BM, H, rows, cols)[0]["uv"]
    return mesh, radius


class Config:
    """kind: 'a' the lit textured colour mesh, 'b' the plain textured mesh, 'c' the lit colour mesh."""

    def __init__(self, R, BM, W, H, rows, cols, tex, kind, persp):
        self.kind = kind
        self.mesh, self.radius = model(BM, H, rows, cols)
        m = self.mesh
        self.ctx = R.RenderContext(W, H, False)
        self.ctx.set_mesh_lights(BL.AMBIENT, BL.LIGHTS)
        self.ctx.set_mesh_perspective(persp)
        if kind == "a":
            self.gm = R.Mesh(m["pos"], m["idx"], colors=m["colors"], uv=m["uv"], normals=m["normals"])
        elif kind == "b":
            self.gm = R.Mesh(m["pos"], m["idx"], uv=m["uv"])
        else:
            self.gm = R.Mesh(m["pos"], m["idx"], colors=m["colors"], gouraud=True, normals=m["normals"])
        self.tex = R.Texture.from_numpy(tex)
        self.mats = [BP.persp_matrix(W, H, self.radius, i) for i in range(360)]
        self.nmats = [BL.normal_matrix(i) for i in range(360)]
        self.begin = BM.begin

    def frame(self, i):
        self.begin(self.ctx)
        k = i % 360
        if self.kind == "a":
            self.ctx.draw_mesh_lit(self.gm, self.mats[k], self.nmats[k], texture=self.tex)
        elif self.kind == "b":
            self.ctx.draw_mesh(self.gm, self.mats[k], texture=self.tex)
        else:
            self.ctx.draw_mesh_lit(self.gm, self.mats[k], self.nmats[k])
        self.ctx.gather_frame_u8()


def verify(R, BM, tex, steps):
    import modulate_ref as M
    import scenes
    W, H = 960, 540
    small = Config(R, BM, W, H, 125, 250, tex, "a", True)
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    k = (steps - 1) % 360
    b = M.mesh_batch(small.mesh, small.mats[k], tex, m=(1.0, 0.0, 0.0, 1.0, 0.0, 0.0), ct=(1.0, 1.0, 1.0, 1.0), lit=True,
                     N=small.nmats[k], ambient=BL.AMBIENT, lights=BL.LIGHTS)
    want = M.expected_payload(W, H, False, BM.BG, "zw", 0xFFFFFFFF, [b])
    return bool(scenes.bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                and small.ctx.last_raster_path() == "order-free")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench_mesh as BM
    import scenes
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("bench_modulate: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    tex = scenes.rng(79).uniform(0, 1, size=(BP.TEX, BP.TEX, 3))
    cfgs = {
        "a1": Config(R, BM, W, H, rows, cols, tex, "a", False),
        "a2": Config(R, BM, W, H, rows, cols, tex, "a", True),
        "b": Config(R, BM, W, H, rows, cols, tex, "b", True),
        "c": Config(R, BM, W, H, rows, cols, tex, "c", True),
    }
    ms = {k: [] for k in cfgs}
    for _ in range(args.pairs):                # alternating groups: a1, a2, b, c, a1, ...
        for k, cfg in cfgs.items():
            ms[k].append(BM.run_timed(cfg, args.steps, args.warmup))
    kern = {k: BL.kernel_times(cfg, args.steps, KERNELS)["tile_raster"] for k, cfg in cfgs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}

    def ratios(x):
        r = [p / q for p, q in zip(ms[x], ms["b"])]
        return dict(median=round(statistics.median(r), 4), pairs=[round(v, 4) for v in r],
                    spread=[round(min(r), 4), round(max(r), 4)])

    res = dict(
        scene="turning C3 sphere, 1M triangles, 1024x1024 RGB texture, perspective matrix, 3840x2160, depth write, "
              "3 directional lights",
        configurations=dict(a1="DrawTexturedMeshLit, mesh perspective off (q == 1)",
                            a2="DrawTexturedMeshLit, mesh perspective on",
                            b="DrawTexturedMesh of the plain textured mesh, mesh perspective on",
                            c="DrawMeshLit of the lit colour mesh"),
        steps=args.steps, pairs=args.pairs,
        ms_per_frame={k: round(v, 4) for k, v in med.items()},
        ms_per_frame_pairs={k: [round(x, 4) for x in v] for k, v in ms.items()},
        raster_us=kern,
        raster_paths={k: cfg.ctx.last_raster_path() for k, cfg in cfgs.items()},
        frame_ratio_a1_over_b=ratios("a1"), frame_ratio_a2_over_b=ratios("a2"),
        raster_ratio_a1_over_b=round(kern["a1"] / kern["b"], 4), raster_ratio_a2_over_b=round(kern["a2"] / kern["b"], 4),
        b_plus_c_ms=round(med["b"] + med["c"], 4),
        b_plus_c_raster_us=round(kern["b"] + kern["c"], 2),
        bar_a_below_b_plus_c=dict(a1=bool(med["a1"] < med["b"] + med["c"]), a2=bool(med["a2"] < med["b"] + med["c"]),
                                  a1_raster=bool(kern["a1"] < kern["b"] + kern["c"]),
                                  a2_raster=bool(kern["a2"] < kern["b"] + kern["c"])),
    )
    if not args.no_verify:
        res["verified"] = verify(R, BM, tex, args.steps)
        res["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles) of a2 against "
                              "tests/modulate_ref.py's expected frame")
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
