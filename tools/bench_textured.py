"""Textured triangles against the paths they stand beside, in one session on
one GPU, by the library's own kernel timing (EnableKernelTiming: the rasters
stamp their execution span on the device clock; the command-list kernel is
timed by events):

  a  the C3 geometry (1M-triangle displaced sphere, 3840x2160) as a Gouraud
     TriangleBuffer -- the existing path, bench.py's frame
  b  the same geometry textured from a 1024x1024 RGB texture, UVs spanning it
     (order-free raster, k_vis)
  c  sprites: 20 000 rotated quads of ~24 px from a 512x512 RGBA atlas at
     1920x1080, as ONE textured batch of 40 000 triangles (ordered raster)
  d  the same sprites as 20 000 DrawSplittedTexture commands in one packed
     ExecuteCommands array inside a command list (one launch)

Ratios: b / a compares two device-clock k_vis spans.  c / d compares GPU time
per frame by HIP events on both sides -- c's binning chain (count, scan, emit,
tile sort) plus its raster against d's one command-list kernel; the raster's
own device-clock span is reported beside it.

Each configuration verifies a frame before it reports: b and c by the
oracle-derived expected frame (tests/textured_ref.py) of a 1/16-size version
of the scene (a quarter of the width and height; c: a sixteenth of the
sprites, same size), d by the oracle on the full frame.  Prints one JSON line
per configuration and writes them all to --out.

    python tools/bench_textured.py --steps 50 --warmup 5 --out profiles/textured/bench_textured.json
    python tools/bench_textured.py --only b,c --no-verify        (for a profiler run)
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BG = (0.0, 0.0, 0.0, 0.0)


def mesh(W, H, rows, cols):
    import scenes
    xy, z, c = scenes.sphere_mesh(W, H, rows, cols)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 6)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 3)
    return xy, np.minimum(z, 0.99), np.ascontiguousarray(c, dtype=np.float64).reshape(xy.shape[0], -1)


def mesh_uv(xy, W, H, tw, th):
    uv = np.empty_like(xy)
    uv[:, 0::2] = xy[:, 0::2] / W * tw
    uv[:, 1::2] = xy[:, 1::2] / H * th
    return uv


def sprites(W, H, n, seed=77, size=24.0, atlas=512, cell=32):
    """n rotated quads: centre, angle, atlas cell -> (xy, uv) of 2n triangles
    and the per-sprite (cx, cy, angle, u0, v0) for the quad commands."""
    g = np.random.default_rng(seed)
    cx, cy = g.uniform(0, W, n), g.uniform(0, H, n)
    ang = g.uniform(0, 2 * math.pi, n)
    cells = atlas // cell
    u0 = g.integers(0, cells, n) * float(cell)
    v0 = g.integers(0, cells, n) * float(cell)
    h = size / 2
    corners = np.array([[-h, -h], [h, -h], [h, h], [-h, h]])
    ca, sa = np.cos(ang), np.sin(ang)
    px = cx[:, None] + corners[None, :, 0] * ca[:, None] - corners[None, :, 1] * sa[:, None]
    py = cy[:, None] + corners[None, :, 0] * sa[:, None] + corners[None, :, 1] * ca[:, None]
    uu = u0[:, None] + np.array([0.0, cell, cell, 0.0])[None, :]
    vv = v0[:, None] + np.array([0.0, 0.0, cell, cell])[None, :]
    tri = np.array([[0, 1, 2], [0, 2, 3]])
    xy = np.stack([px[:, tri], py[:, tri]], axis=-1).reshape(2 * n, 6)
    uv = np.stack([uu[:, tri], vv[:, tri]], axis=-1).reshape(2 * n, 6)
    return xy, uv, (cx, cy, ang, u0, v0)


def atlas_texture(size=512, seed=78):
    g = np.random.default_rng(seed)
    t = g.uniform(0, 1, size=(size, size, 4))
    t[..., 3] = g.uniform(0.3, 1.0, size=(size, size))
    return t


def timed(ctx, name, frame, steps, warmup):
    for i in range(warmup):
        frame()
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter(name)
    ctx.enable_kernel_timing(True)
    for i in range(steps):
        frame()
    ctx.flush()
    ctx.enable_kernel_timing(False)
    tot, cnt = ctx.get_kernel_timing(name)
    ctx.reset_kernel_timing()
    if not cnt:
        raise SystemExit(f"bench_textured: no launch of '{name}' was timed")
    return tot / cnt * 1e3, cnt


def same(got, want):
    import scenes
    return bool(scenes.bits_equal(got[0], want[0]) and (want[1] is None or np.array_equal(got[1], want[1])))


def config_a(R, args):
    W, H = 3840, 2160
    xy, z, c = mesh(W, H, 500, 1000)
    ctx = R.RenderContext(W, H, False)
    buf = R.TriangleBuffer(xy, c, z=z, gouraud=True)

    def frame():
        ctx.set_color(*BG)
        ctx.set_depth_state(True, True)
        ctx.clear_depth()
        ctx.draw_triangle_buffer(buf)
        ctx.gather_frame_u8()
    us, cnt = timed(ctx, "tile_raster", frame, args.steps, args.warmup)
    return dict(config="a: C3 geometry, Gouraud TriangleBuffer (existing path)", W=W, H=H, triangles=len(xy),
                raster_path=ctx.last_raster_path(), k_vis_us=round(us, 2), launches=cnt,
                warm_failures=int(ctx.warm_failure_count()), verified=None,
                verify_note="bench.py verifies this frame against the oracle's digests")


def config_b(R, args):
    import scenes
    import textured_ref as T
    W, H, tw = 3840, 2160, 1024
    tex = scenes.rng(79).uniform(0, 1, size=(tw, tw, 3))
    out = dict(config="b: C3 geometry textured from a 1024x1024 RGB texture", W=W, H=H)
    if not args.no_verify:   # 1/16-size version: 960x540, a 125x250 mesh, UVs spanning the same texture
        sw, sh = W // 4, H // 4
        sxy, sz, _ = mesh(sw, sh, 125, 250)
        b = dict(xy=sxy, uv=mesh_uv(sxy, sw, sh, tw, tw), z=sz, tex=tex, ct=(1.0, 1.0, 1.0, 1.0), m=T.IDENT)
        want = T.expected_payload(sw, sh, False, BG, "zw", 0xFFFFFFFF, [b])
        small = R.RenderContext(sw, sh, False)
        got = T.draw_gpu(small, scenes.GpuFactory(), "zw", 0xFFFFFFFF, BG, [b])
        out["verified"] = same(got, want) and small.last_raster_path() == "order-free"
        out["verify_note"] = "1/16-size scene (960x540, 62 500 triangles) against the oracle-derived frame"
    xy, z, _ = mesh(W, H, 500, 1000)
    ctx = R.RenderContext(W, H, False)
    gtex = R.Texture.from_numpy(tex)
    buf = R.TriangleBuffer(xy, uv=mesh_uv(xy, W, H, tw, tw), z=z)

    def frame():
        ctx.set_color(*BG)
        ctx.set_depth_state(True, True)
        ctx.clear_depth()
        ctx.draw_triangle_buffer(buf, gtex)
        ctx.gather_frame_u8()
    us, cnt = timed(ctx, "tile_raster", frame, args.steps, args.warmup)
    out.update(triangles=len(xy), raster_path=ctx.last_raster_path(), k_vis_us=round(us, 2), launches=cnt,
               warm_failures=int(ctx.warm_failure_count()))
    return out


def config_c(R, args):
    import scenes
    import textured_ref as T
    W, H, n = 1920, 1080, 20000
    atlas = atlas_texture()
    out = dict(config="c: 20 000 rotated 24 px sprites from a 512x512 RGBA atlas, one textured batch", W=W, H=H)
    if not args.no_verify:
        sw, sh = W // 4, H // 4
        sxy, suv, _ = sprites(sw, sh, n // 16)
        b = dict(xy=sxy, uv=suv, z=None, tex=atlas, ct=(1.0, 1.0, 1.0, 1.0), m=T.IDENT)
        want = T.expected_loop(sw, sh, False, BG, "nz", 0, [b])
        small = R.RenderContext(sw, sh, False)
        got = T.draw_gpu(small, scenes.GpuFactory(), "nz", 0, BG, [b])
        out["verified"] = same(got, want) and small.last_raster_path() == "ordered"
        out["verify_note"] = "1/16-size scene (480x270, 1250 sprites) against the oracle-derived frame"
    xy, uv, _ = sprites(W, H, n)
    ctx = R.RenderContext(W, H, False)
    gtex = R.Texture.from_numpy(atlas)
    buf = R.TriangleBuffer(xy, uv=uv)

    def frame():
        ctx.set_color(*BG)
        ctx.set_depth_state(False, False)
        ctx.draw_triangle_buffer(buf, gtex)
        ctx.gather_frame_u8()
    us, cnt = timed(ctx, "tile_raster", frame, args.steps, args.warmup)
    binning = {}
    for i in range(3):
        frame()
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    ctx.enable_kernel_timing(True)
    for i in range(args.steps):
        frame()
    ctx.flush()
    ctx.enable_kernel_timing(False)
    for name in ("tri_count", "tri_scan", "tri_emit", "tri_sort", "tile_raster"):
        tot, k = ctx.get_kernel_timing(name)
        if k:
            binning[name] = round(tot / k * 1e3, 2)
    out.update(triangles=len(xy), raster_path=ctx.last_raster_path(), tile_raster_us=round(us, 2), launches=cnt,
               kernels_us_event_timed=binning, gpu_us_event_timed=round(sum(binning.values()), 2))
    return out


def config_d(R, args):
    import scenes
    W, H, n = 1920, 1080, 20000
    atlas = atlas_texture()
    _, _, (cx, cy, ang, u0, v0) = sprites(W, H, n)
    size, cell, asz = 24.0, 32.0, 512.0

    def draw(c, tex):
        for k in range(n):
            c.save_state()
            c.translate(float(cx[k]), float(cy[k]))
            c.rotate(float(ang[k]))
            c.draw_splitted_texture(tex, -size / 2, -size / 2, size, size, float(u0[k]) / asz,
                                    float(u0[k] + cell) / asz, float(v0[k]) / asz, float(v0[k] + cell) / asz)
            c.restore_state()

    ctx = R.RenderContext(W, H, False)
    gtex = R.Texture.from_numpy(atlas)
    ctx.begin_commands()
    packed = ctx.packed()

    def frame():
        packed.set_color(*BG)
        draw(packed, gtex)
        packed.submit()
        ctx.flush_commands()
    out = dict(config="d: the same sprites as 20 000 DrawSplittedTexture commands in one ExecuteCommands array",
               W=W, H=H, commands=n)
    if not args.no_verify:
        frame()
        got = ctx.get_buffer_numpy()
        ofac = scenes.OracleFactory()
        octx = ofac.context(W, H, False)
        octx.set_color(*BG)
        draw(octx, ofac.texture(atlas))
        out["verified"] = bool(scenes.bits_equal(got, octx.get_buffer_numpy()))
        out["verify_note"] = "the full frame against the oracle"
    steps = max(3, args.steps // 5)   # (packing 20 000 commands in Python dominates the wall time)
    us, cnt = timed(ctx, "prim", frame, steps, 2)
    out.update(cmd_list_kernel_us=round(us, 2), launches=cnt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    if R.device_count() <= 0:
        raise SystemExit("bench_textured: no HIP device")
    R.set_device(0)
    results = {}
    for key, fn in (("a", config_a), ("b", config_b), ("c", config_c), ("d", config_d)):
        if key in args.only.split(","):
            results[key] = fn(R, args)
            print(json.dumps(results[key]), flush=True)
    if "a" in results and "b" in results:
        results["b_over_a_k_vis"] = round(results["b"]["k_vis_us"] / results["a"]["k_vis_us"], 3)
    if "c" in results and "d" in results:
        # events on both sides: c's binning + raster against d's command-list kernel
        results["c_over_d_gpu_time_event_timed"] = round(results["c"]["gpu_us_event_timed"] /
                                                         results["d"]["cmd_list_kernel_us"], 3)
    print(json.dumps({k: v for k, v in results.items() if not isinstance(v, dict)}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
