"""An animated mesh, posed every frame: what skinning on the device costs beside
the only route there was before it, in one session on one GPU.

The workload is a UV sphere of 224 x 448 = 100 352 vertices (199 362 triangles,
Gouraud, depth write, 1920x1080) under a rig of 64 bones; a frame is the clears,
a new pose and one draw_mesh, and a run is N frames with one flush at the end.

  a  update_positions with the pose precomputed in numpy (the host arithmetic is
     not counted), then the draw: a pipeline drain, an upload of nv*3 doubles and
     a stream wait per frame
  b  pose_mesh with the frame's palette (64 x 12 doubles), then the draw: one
     asynchronous copy of 6 KB and one kernel, no host wait

a and b alternate over --rounds rounds in one process; each line is wall-clock ms
per frame (host clock around frames that end in a flush) after a clock settle and
a warmup, the median round with all rounds listed.

The skin kernel's own time is the library's kernel timing of `mesh_skin` (HIP
events around each launch, so every figure includes the launch gap), for each
kernel variant -- the palette read from global memory (1) and staged in LDS (2)
-- alternating, the global one twice for its run-to-run spread, on the coherent
rig (a vertex blends four neighbouring height bands) and on a random one (four
random bones per vertex).  It is set against the time its bytes take at 6.3 TB/s:
72 B in and 24 B out per vertex for the positions.

b's last frame is compared bit for bit with a's (the same pose index).  Prints one
JSON line per result and writes them all to --out.

    python tools/skin_bench.py --steps 200 --warmup 20 --out profiles/skin/skin_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_mesh as BM   # noqa: E402  (the sphere, the clears and the timing loop)

HBM_TBS = BM.HBM_TBS
W, H, ROWS, COLS, NB, POSES = 1920, 1080, 223, 447, 64, 48


def rig(mesh, radius, kind, seed=3):
    """(joints (nv, 4) uint32, weights (nv, 4)): `coherent` -- bone b owns the height band b of NB, a vertex blends
    the bands b - 1 .. b + 2 around its own by distance; `random` -- four random bones and weights per vertex."""
    nv = mesh["pos"].shape[0]
    g = np.random.default_rng(seed)
    if kind == "random":
        joints = g.integers(0, NB, size=(nv, 4))
        w = g.uniform(0.05, 1.0, size=(nv, 4))
    else:
        t = (mesh["pos"][:, 1] / (1.15 * radius) * 0.5 + 0.5) * (NB - 1)
        b = np.clip(np.floor(t).astype(np.int64), 0, NB - 1)
        joints = np.clip(b[:, None] + np.array([0, 1, -1, 2])[None, :], 0, NB - 1)
        w = 1.0 / (0.25 + np.abs(joints - t[:, None]))
    return np.ascontiguousarray(joints.astype(np.uint32)), np.ascontiguousarray(w / w.sum(axis=1)[:, None])


def palette(frame, radius):
    """(NB, 12): bone b turns about the y axis and sways sideways, by an amount that grows with its height and the frame."""
    b = np.arange(NB)
    a = 0.012 * (b - NB / 2) * np.sin(0.13 * frame + 0.05 * b)
    c, s = np.cos(a), np.sin(a)
    pal = np.zeros((NB, 3, 4))
    pal[:, 0, 0], pal[:, 0, 2], pal[:, 1, 1], pal[:, 2, 0], pal[:, 2, 2] = c, s, 1.0, -s, c
    pal[:, 0, 3] = 0.04 * radius * np.sin(0.21 * frame + 0.2 * b)
    return np.ascontiguousarray(pal.reshape(NB, 12))


class Config:
    def __init__(self, R, route, kind="coherent"):
        import mesh_skin_ref as MS
        self.route = route
        self.mesh, self.radius = BM.model(H, ROWS, COLS)
        self.joints, self.weights = rig(self.mesh, self.radius, kind)
        self.ctx = R.RenderContext(W, H, False)
        self.gm = R.Mesh(self.mesh["pos"], self.mesh["idx"], colors=self.mesh["colors"], gouraud=True)
        self.M = BM.matrix(W, H, self.radius, 20)
        self.pals = [palette(i, self.radius) for i in range(POSES)]
        if route == "a":
            self.name = "a: update_positions with a precomputed numpy pose, then draw_mesh"
            self.poses = [MS.pose(self.mesh["pos"], None, self.joints, self.weights, p)[0] for p in self.pals]
        else:
            self.name = "b: pose_mesh with the frame's palette, then draw_mesh"
            self.skin = R.MeshSkin(self.mesh["pos"], self.joints, self.weights, NB)

    def frame(self, i):
        BM.begin(self.ctx)
        if self.route == "a":
            self.gm.update_positions(self.poses[i % POSES])
        else:
            self.ctx.pose_mesh(self.gm, self.skin, self.pals[i % POSES])
        self.ctx.draw_mesh(self.gm, self.M)


def skin_kernel_us(cfg, variant, steps):
    """us per launch of the skin kernel of `variant` over `steps` frames of b (event-timed)."""
    ctx = cfg.ctx
    cfg.skin.set_variant(variant)
    for i in range(5):
        cfg.frame(i)
    ctx.flush()
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("mesh_skin")
    ctx.enable_kernel_timing(True)
    for i in range(steps):
        cfg.frame(i)
    ctx.flush()
    ctx.enable_kernel_timing(False)
    tot, cnt = ctx.get_kernel_timing("mesh_skin")
    if cnt != steps:
        raise SystemExit(f"skin_bench: {cnt} launches of mesh_skin were timed, not {steps}")
    ctx.reset_kernel_timing()
    ctx.set_kernel_timing_filter("")
    cfg.skin.set_variant(0)
    return round(tot / cnt * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from libnativecpurenderer_amd import libNativeCPURendererPybind as R
    import scenes
    if R.device_count() <= 0:
        raise SystemExit("skin_bench: no HIP device")
    R.set_device(0)
    cfgs = {"a": Config(R, "a"), "b": Config(R, "b")}
    nv, n = cfgs["a"].mesh["pos"].shape[0], cfgs["a"].mesh["idx"].shape[0]
    rounds = {k: [] for k in cfgs}
    for _ in range(args.rounds):                            # alternating: a, b, a, b, ...
        for k, cfg in cfgs.items():
            rounds[k].append(BM.run_timed(cfg, args.steps, args.warmup))
    results = {}
    for k, cfg in cfgs.items():
        results[k] = dict(config=cfg.name, W=W, H=H, vertices=nv, triangles=n, bones=NB, steps=args.steps,
                          ms_per_frame=round(statistics.median(rounds[k]), 4),
                          ms_per_frame_rounds=[round(v, 4) for v in rounds[k]])
        print(json.dumps(results[k]), flush=True)
    results["a_over_b"] = round(results["a"]["ms_per_frame"] / results["b"]["ms_per_frame"], 2)
    # the same pose index on both routes: the same frame, bit for bit
    last = args.steps - 1
    frames = {}
    for k, cfg in cfgs.items():
        cfg.frame(last)
        frames[k] = (cfg.ctx.get_buffer_numpy(), cfg.ctx.get_depth_buffer())
    results["b_frame_equals_a_frame"] = bool(scenes.bits_equal(frames["a"][0], frames["b"][0])
                                             and np.array_equal(frames["a"][1], frames["b"][1]))
    # the skin kernel: global, LDS, global, LDS, ... per rig
    nbytes = 96 * nv
    bound_us = round(nbytes / (HBM_TBS * 1e12) * 1e6, 3)
    kern = dict(bytes_per_launch=nbytes, bound_us_at_6_3_TBs=bound_us, palette_bytes=NB * 96, note=(
        "us per launch from HIP events around each launch (includes the launch gap); bytes: 24 B position, "
        "16 B joints, 32 B weights in and 24 B out per vertex, the palette not counted"))
    for kind in ("coherent", "random"):
        cfg = cfgs["b"] if kind == "coherent" else Config(R, "b", kind)
        runs = {"global": [], "lds": []}
        for _ in range(max(2, args.rounds)):
            runs["global"].append(skin_kernel_us(cfg, 1, args.steps))
            runs["lds"].append(skin_kernel_us(cfg, 2, args.steps))
        g, l = statistics.median(runs["global"]), statistics.median(runs["lds"])
        kern[kind] = dict(global_us=runs["global"], lds_us=runs["lds"], global_median_us=g, lds_median_us=l,
                          global_spread_us=round(max(runs["global"]) - min(runs["global"]), 3),
                          global_minus_lds_us=round(g - l, 3),
                          bound_over_global=round(bound_us / g, 3), bound_over_lds=round(bound_us / l, 3))
    results["skin_kernel"] = kern
    print(json.dumps({k: v for k, v in results.items() if k not in cfgs}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    t0 = time.perf_counter()
    main()
    print(f"skin_bench: {time.perf_counter() - t0:.1f} s", flush=True)
