"""What wrap addressing costs: tools/bench_filter.py's scene (the turning C3
sphere: 501 x 1001 vertices, 1M triangles, depth write, 3840x2160, a new
perspective matrix every frame, SetMeshPerspective on) drawing a 128 x 128 RGB
texture with the UVs scaled to tile it 8 x 8, with SetTriangleTextureWrap (0, 0)
and (1, 1) -- the same frames, in one process on one GPU, in interleaved pairs
(clamp, repeat, clamp, repeat, ...) -- with the filter off and with it on:

  (0, 0)  the clamp samplers (tex_index / tex_bilinear): past the first tile
          every coordinate clamps to the border texels
  (1, 1)  wrap_fold per axis: an IEEE f64 divide, a floor, a product, a
          difference and a few compares per axis and shaded pixel; the four
          texels of a bilinear footprint by a base offset and two signed strides

Wall-clock ms per frame (host clock around frames that end in a flush) after a
clock settle and warmup, the median pair and the spread of the pairs; then the
library's kernel timing (GetKernelTiming) of the raster (k_vis, stamped on the
device clock) in each state.  Reported per filter state: the ratio repeat /
clamp of the frame and of the raster.  The two states read different texels
(the clamped frame reads the border texels only), so the ratio holds the
arithmetic and the difference in texture locality together.

The last timed frame of a 1/16-size version (960x540, a 125 x 250 mesh) under
(1, 1) is verified against tests/wrap_ref.py's expected frame, in both filter
states.

    python tools/bench_wrap.py --steps 40 --warmup 5 --out profiles/wrap/ab_bench.json
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

import bench_persp as BP   # noqa: E402  (the scene: Config, the matrices, kernel_times)

TEX, TILES = 128, 8


class Config(BP.Config):
    """bench_persp's configuration with the mesh's UVs running over TILES x TILES copies of the texture."""

    def __init__(self, R, BM, W, H, rows, cols, tex, filt, wrap):
        super().__init__(R, BM, W, H, rows, cols, tex, True)
        self.mesh = dict(self.mesh, uv=np.ascontiguousarray(self.mesh["uv"] * (TILES * TEX / (BP.TEX - 1.0))))
        self.gm = R.Mesh(self.mesh["pos"], self.mesh["idx"], uv=self.mesh["uv"])
        self.ctx.set_triangle_texture_filter(filt)
        self.ctx.set_triangle_texture_wrap(*wrap)


def verify(R, BM, tex, steps, filt):
    import persp_ref as P
    import scenes
    import wrap_ref as WR
    W, H = 960, 540
    small = Config(R, BM, W, H, 125, 250, tex, filt, (1, 1))
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    b = P.mesh_batch(small.mesh, small.mats[(steps - 1) % 360], tex, persp=True, m=(1.0, 0.0, 0.0, 1.0, 0.0, 0.0),
                     ct=(1.0, 1.0, 1.0, 1.0))
    want = WR.expected_payload(W, H, False, BM.BG, "zw", 0xFFFFFFFF, [b], filt=filt, wrap=(1, 1))
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
        raise SystemExit("bench_wrap: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    tex = scenes.rng(79).uniform(0, 1, size=(TEX, TEX, 3))
    res = dict(
        scene=("turning C3 sphere, 1M triangles, 128x128 RGB texture tiled 8 x 8 by the UVs, perspective matrix, "
               "mesh perspective on, 3840x2160, depth write"),
        steps=args.steps, pairs=args.pairs, states={})
    names = {(0, 0): "clamp", (1, 1): "repeat"}
    for filt in (0, 1):
        cfgs = {w: Config(R, BM, W, H, rows, cols, tex, filt, w) for w in names}
        ms = {w: [] for w in names}
        for p in range(args.pairs):            # interleaved pairs: clamp, repeat, clamp, repeat, ...
            for w in names:
                ms[w].append(BM.run_timed(cfgs[w], args.steps, args.warmup))
        kern = {w: BP.kernel_times(cfgs[w], args.steps) for w in names}
        med = {w: statistics.median(v) for w, v in ms.items()}
        ratios = [b / a for a, b in zip(ms[(0, 0)], ms[(1, 1)])]
        st = dict(
            ms_per_frame={names[w]: round(med[w], 4) for w in med},
            ms_per_frame_pairs={names[w]: [round(v, 4) for v in ms[w]] for w in ms},
            frame_ratio_repeat_over_clamp=round(statistics.median(ratios), 4),
            frame_ratio_pairs=[round(r, 4) for r in ratios],
            frame_ratio_spread=[round(min(ratios), 4), round(max(ratios), 4)],
            kernels_us={names[w]: kern[w] for w in kern},
            raster_ratio_repeat_over_clamp=round(kern[(1, 1)]["tile_raster"] / kern[(0, 0)]["tile_raster"], 4),
            frame_difference_us=round((med[(1, 1)] - med[(0, 0)]) * 1e3, 2),
            raster_difference_us=round(kern[(1, 1)]["tile_raster"] - kern[(0, 0)]["tile_raster"], 2),
            raster_path=cfgs[(1, 1)].ctx.last_raster_path(),
        )
        if not args.no_verify:
            st["verified"] = verify(R, BM, tex, args.steps, filt)
        res["states"][f"filter{filt}"] = st
        del cfgs
    if not args.no_verify:
        res["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles), wrap (1, 1), "
                              "against tests/wrap_ref.py's expected frame")
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
