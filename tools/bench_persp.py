"""What perspective-correct texture mapping costs: the turning C3 sphere
(tools/bench_mesh.py's mesh: 501 x 1001 vertices, 1M triangles, depth write,
3840x2160) textured from a 1024x1024 RGB texture under a perspective matrix, a
new one every frame, with SetMeshPerspective off and on -- the same frames, in
one process on one GPU, in interleaved pairs (off, on, off, on, ...):

  off  the vertex stage drops cw: UVs affine in screen space (ATTR_TEX)
  on   q = 1 / cw per vertex, gathered like z; the rasters sample at
       (U / Q, V / Q) (ATTR_TEX_PERSP): one IEEE division and five more
       products per shaded pixel, three more doubles per triangle record

Wall-clock ms per frame (host clock around frames that end in a flush) after a
clock settle and warmup, the median pair and the spread; then the library's
kernel timing (GetKernelTiming) of the vertex stage, the assembly and the
raster (k_vis, stamped on the device clock) in each state.  Reported: the
ratio on / off of the frame and of the raster, and the raster's share of the
frame's difference.

The last timed frame of a 1/16-size version (960x540, a 125 x 250 mesh) with
the state on is verified against tests/persp_ref.py's expected frame.

    python tools/bench_persp.py --steps 40 --warmup 5 --out profiles/persp/ab_bench.json
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

KERNELS = ("mesh_vertex", "mesh_assemble", "tile_raster")
TEX = 1024


def persp_matrix(W, H, R, frame):
    """Frame `frame`'s matrix: the eye 3 R in front of the sphere's centre, the
    model turning as in bench_mesh.matrix; cw = the view-space depth in pixels
    (1.8 R .. 4.2 R over the sphere), z from 0.05 to 0.95 over that range."""
    a, b = np.radians(1.0 + frame), np.radians(0.5 * frame)
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    ry = np.array([[ca, 0, sa, 0], [0, 1, 0, 0], [-sa, 0, ca, 0], [0, 0, 0, 1.0]])
    rx = np.array([[1, 0, 0, 0], [0, cb, -sb, 0], [0, sb, cb, 0], [0, 0, 0, 1.0]])
    view = rx @ ry
    view[2, 3] = 3.0 * R
    near, far = 1.8 * R, 4.2 * R
    zb = (0.95 - 0.05) / (1 / far - 1 / near)
    za = 0.05 - zb / near
    s = 0.5 * H * 2.4
    proj = np.array([[s, 0, W / 2, 0], [0, -s, H / 2, 0], [0, 0, za, zb], [0, 0, 1.0, 0]])
    return np.ascontiguousarray((proj @ view).reshape(16))


def textured_model(BM, H, rows, cols):
    mesh, radius = BM.model(H, rows, cols)
    th = np.linspace(0, 1, rows + 1)
    ph = np.linspace(0, 1, cols + 1)
    Tm, Pm = np.meshgrid(th, ph, indexing="ij")
    uv = np.stack([Pm * (TEX - 1), Tm * (TEX - 1)], -1).reshape(-1, 2)
    return dict(pos=mesh["pos"], idx=mesh["idx"], uv=np.ascontiguousarray(uv)), radius


class Config:
    def __init__(self, R, BM, W, H, rows, cols, tex, on):
        self.W, self.H, self.on = W, H, on
        self.mesh, self.radius = textured_model(BM, H, rows, cols)
        self.ctx = R.RenderContext(W, H, False)
        self.gm = R.Mesh(self.mesh["pos"], self.mesh["idx"], uv=self.mesh["uv"])
        self.tex = R.Texture.from_numpy(tex)
        self.mats = [persp_matrix(W, H, self.radius, i) for i in range(360)]
        self.ctx.set_mesh_perspective(on)
        self.begin = BM.begin

    def frame(self, i):
        self.begin(self.ctx)
        self.ctx.draw_mesh(self.gm, self.mats[i % 360], texture=self.tex)
        self.ctx.gather_frame_u8()


def kernel_times(cfg, steps):
    ctx = cfg.ctx
    for i in range(3):
        cfg.frame(i)
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter(",".join(KERNELS))
    ctx.enable_kernel_timing(True)
    for i in range(steps):
        cfg.frame(i)
    ctx.flush()
    ctx.enable_kernel_timing(False)
    out = {}
    for name in KERNELS:
        tot, cnt = ctx.get_kernel_timing(name)
        if not cnt:
            raise SystemExit(f"bench_persp: no launch of '{name}' was timed")
        out[name] = round(tot / cnt * 1e3, 2)
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    return out


def verify(R, BM, tex, steps):
    import persp_ref as P
    import scenes
    W, H = 960, 540
    small = Config(R, BM, W, H, 125, 250, tex, True)
    for i in range(steps):
        small.frame(i)
    got = small.ctx.get_buffer_numpy(), small.ctx.get_depth_buffer()
    b = P.mesh_batch(small.mesh, small.mats[(steps - 1) % 360], tex, m=(1.0, 0.0, 0.0, 1.0, 0.0, 0.0),
                     ct=(1.0, 1.0, 1.0, 1.0))
    want = P.expected_payload(W, H, False, BM.BG, "zw", 0xFFFFFFFF, [b])
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
        raise SystemExit("bench_persp: no HIP device")
    R.set_device(0)
    W, H, rows, cols = 3840, 2160, 500, 1000
    tex = scenes.rng(79).uniform(0, 1, size=(TEX, TEX, 3))
    cfgs = {"off": Config(R, BM, W, H, rows, cols, tex, False), "on": Config(R, BM, W, H, rows, cols, tex, True)}
    ms = {"off": [], "on": []}
    for p in range(args.pairs):            # interleaved pairs: off, on, off, on, ...
        for k in ("off", "on"):
            ms[k].append(BM.run_timed(cfgs[k], args.steps, args.warmup))
    kern = {k: kernel_times(cfgs[k], args.steps) for k in ("off", "on")}
    med = {k: statistics.median(v) for k, v in ms.items()}
    pair_ratios = [b / a for a, b in zip(ms["off"], ms["on"])]
    d_frame_us = (med["on"] - med["off"]) * 1e3
    d_raster_us = kern["on"]["tile_raster"] - kern["off"]["tile_raster"]
    res = dict(
        scene="turning C3 sphere, 1M triangles, 1024x1024 RGB texture, perspective matrix, 3840x2160, depth write",
        steps=args.steps, pairs=args.pairs,
        ms_per_frame={k: round(med[k], 4) for k in med},
        ms_per_frame_pairs={k: [round(v, 4) for v in ms[k]] for k in ms},
        frame_ratio_on_over_off=round(statistics.median(pair_ratios), 4),
        frame_ratio_pairs=[round(r, 4) for r in pair_ratios],
        kernels_us={k: kern[k] for k in kern},
        raster_ratio_on_over_off=round(kern["on"]["tile_raster"] / kern["off"]["tile_raster"], 4),
        frame_difference_us=round(d_frame_us, 2),
        raster_difference_us=round(d_raster_us, 2),
        raster_share_of_frame_difference=(round(d_raster_us / d_frame_us, 3) if abs(d_frame_us) > 1e-9 else None),
        raster_path=cfgs["on"].ctx.last_raster_path(),
    )
    if not args.no_verify:
        res["verified"] = verify(R, BM, tex, args.steps)
        res["verify_note"] = ("the last timed frame of the 1/16-size scene (960x540, 62 500 triangles), state on, "
                              "against tests/persp_ref.py's expected frame")
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
