"""What the bilinear texture filter costs: tools/bench_persp.py's scene (the
turning C3 sphere: 501 x 1001 vertices, 1M triangles, depth write, 3840x2160,
a 1024x1024 RGB texture, a new perspective matrix every frame) drawn with
SetTriangleTextureFilter 0 and 1 -- the same frames, in one process on one
GPU, in interleaved pairs (0, 1, 0, 1, ...) -- with SetMeshPerspective off and
with it on:

  filter 0  one texel per shaded pixel (24 B), tex_index
  filter 1  four texels (two adjacent pairs, a row apart: 96 B), two fractions
            and 9 products + 3 additions per channel, one pixel's gathers in
            flight per thread instead of two

Wall-clock ms per frame (host clock around frames that end in a flush) after a
clock settle and warmup, the median pair and the spread of the pairs; then the
library's kernel timing (GetKernelTiming) of the raster (k_vis, stamped on the
device clock) in each state.  Reported per perspective state: the ratio filter
1 / filter 0 of the frame and of the raster.

The last timed frame of a 1/16-size version (960x540, a 125 x 250 mesh) with
the filter on is verified against tests/bilinear_ref.py's expected frame, in
both perspective states.

    python tools/bench_filter.py --steps 40 --warmup 5 --out profiles/bilinear/ab_bench.json
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


def config(R, BM, W, H, rows, cols, tex, persp, filt):
    cfg = BP.Config(R, BM, W, H, rows, cols, tex, persp)
    cfg.ctx.set_triangle_texture_filter(filt)
    return cfg


def verify(R, BM, tex, steps, persp):
    import bilinear_ref as B
    import persp_ref as P
    import scenes
    W, H = 960, 540
    small = config(R, BM, W, H, 125, 250, tex, persp, 1)
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    b = P.mesh_batch(small.mesh, small.mats[(steps - 1) % 360], tex, persp=persp, m=(1.0, 0.0, 0.0, 1.0, 0.0, 0.0),
                     ct=(1.0, 1.0, 1.0, 1.0))
    want = B.expected_payload(W, H, False, BM.BG, "zw", 0xFFFFFFFF, [b])
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
        raise SystemExit("bench_filter: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    tex = scenes.rng(79).uniform(0, 1, size=(BP.TEX, BP.TEX, 3))
    res = dict(
        scene="turning C3 sphere, 1M triangles, 1024x1024 RGB texture, perspective matrix, 3840x2160, depth write",
        steps=args.steps, pairs=args.pairs, states={})
    for persp in (False, True):
        cfgs = {f: config(R, BM, W, H, rows, cols, tex, persp, f) for f in (0, 1)}
        ms = {0: [], 1: []}
        for p in range(args.pairs):            # interleaved pairs: 0, 1, 0, 1, ...
            for f in (0, 1):
                ms[f].append(BM.run_timed(cfgs[f], args.steps, args.warmup))
        kern = {f: BP.kernel_times(cfgs[f], args.steps) for f in (0, 1)}
        med = {f: statistics.median(v) for f, v in ms.items()}
        ratios = [b / a for a, b in zip(ms[0], ms[1])]
        st = dict(
            ms_per_frame={f"filter{f}": round(med[f], 4) for f in med},
            ms_per_frame_pairs={f"filter{f}": [round(v, 4) for v in ms[f]] for f in ms},
            frame_ratio_1_over_0=round(statistics.median(ratios), 4),
            frame_ratio_pairs=[round(r, 4) for r in ratios],
            frame_ratio_spread=[round(min(ratios), 4), round(max(ratios), 4)],
            kernels_us={f"filter{f}": kern[f] for f in kern},
            raster_ratio_1_over_0=round(kern[1]["tile_raster"] / kern[0]["tile_raster"], 4),
            frame_difference_us=round((med[1] - med[0]) * 1e3, 2),
            raster_difference_us=round(kern[1]["tile_raster"] - kern[0]["tile_raster"], 2),
            raster_path=cfgs[1].ctx.last_raster_path(),
        )
        if not args.no_verify:
            st["verified"] = verify(R, BM, tex, args.steps, persp)
        res["states"]["mesh_perspective_on" if persp else "mesh_perspective_off"] = st
        del cfgs
    if not args.no_verify:
        res["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles), filter 1, "
                              "against tests/bilinear_ref.py's expected frame")
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
