"""Per-phase clocks of the steady raster's work items (probe build: NR_LIB=tools/exp/probe.so, built with
`make LIB=tools/exp/probe.so OBJ=/tmp/obj_probe EXTRA=-DNR_PROBE=1`), by item-length class.

Renders FRAMES frames of a bench configuration (optionally one shard of N) with a drain after each, so the host sees
every stage of the schedule generation complete (cold, warm, marking, pruned, capture, cached), clears the probe, renders
one more frame and prints, for that frame's items: key init (item start -> stamp 1), raster (1 -> 2), hash insert
(2 -> 4), record build (4 -> 5), pixel pass and stores (5 -> item end).  k_keys stamps 1 and 2 together once the cached
keys are in LDS, so its "key init" is the key load and its raster is zero.

Run from the repository root (the tree whose bench.py and package are to be used):
    NR_LIB=tools/exp/probe.so python tools/exp/key_phases.py [config] [shards] [frames] [frame]
"frame": the probed frame is the steady frame of bench.py -- the frame output on, SetDeferredStores(1), no readback,
so a cached Gouraud batch runs its frame-only (KO_FRAME) instance."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.getcwd()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from libnativecpurenderer_amd import _lib  # noqa: E402
if os.environ.get("NR_LIB"):   # (tools only: the probe build instead of the shipped library)
    _lib.LIB_PATH = os.path.abspath(os.environ["NR_LIB"])
from libnativecpurenderer_amd import libNativeCPURendererPybind as R  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
shards = int(sys.argv[2]) if len(sys.argv) > 2 else 1
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 10
steady = len(sys.argv) > 4 and sys.argv[4] == "frame"
cfg = bench.CONFIGS[name]
xy, z, c = bench.make_scene(cfg)
ctx = R.RenderContext(cfg["W"], cfg["H"], False)
if shards > 1:
    ctx.set_shard(shards, 0)
buf = R.TriangleBuffer(xy, c, z=z, gouraud=cfg["gouraud"])
lib = _lib.load()
lib.NrProbeReset.restype = None
lib.NrProbeRead.restype = ctypes.c_long
lib.NrProbeRead.argtypes = [ctypes.c_void_p, ctypes.c_long]


if steady:
    ctx.set_deferred_stores(1)
    ctx.set_frame_format("yuv420p")
    ctx.gather_frame_u8()


def frame(read=True):
    ctx.set_color(0, 0, 0, 0)
    ctx.set_depth_state(True, cfg.get("write", True))
    ctx.clear_depth()
    ctx.draw_triangle_buffer(buf)
    ctx.flush()
    if read:
        ctx.get_depth_buffer()   # (a readback: the device is drained and the host polls its stages at the next draw)


for _ in range(frames):
    frame()
lib.NrProbeReset()
frame(read=not steady)
out = np.zeros(65536 * 8, np.uint64)
n = lib.NrProbeRead(out.ctypes.data, 65536)
e = out[: 8 * n].reshape(n, 8)
nt = (e[:, 0] >> 32).astype(np.int64)
L = ((e[:, 2] >> 32) - (e[:, 2] & 0xFFFFFFFF)).astype(np.int64)
nsl = ((e[:, 1] >> 32) & 0xFFFF).astype(np.int64)
dur = (e[:, 3] & 0xFFFFFF).astype(np.float64) / 100.0
t0 = (e[:, 3] >> 24).astype(np.float64) / 100.0
span = (t0 + dur).max() - t0.min()
ph = np.stack([((e[:, 4] >> (16 * q)) & 0xFFFF) for q in range(4)] + [(e[:, 5] >> (16 * q)) & 0xFFFF for q in range(3)],
              1).astype(np.float64)
ph[(ph == 0xFFFF) | (ph == 0)] = np.nan
ph /= 100.0
keys, ras, mrg, hsh, rec = ph[:, 0], ph[:, 1], ph[:, 2], ph[:, 3], ph[:, 4]
counts = {k: getattr(ctx, k)() for k in ("pruned_batch_count", "replanned_batch_count") if hasattr(ctx, k)}
if hasattr(ctx, "key_cached_batch_count"):
    counts["key_cached_batch_count"] = ctx.key_cached_batch_count()
print(f"{name} shards={shards}: frame {frames} after {frames} drained frames; {counts}")
print(f"{n} items, workgroup size {sorted(set(nt.tolist()))}, span {span:.1f} us, sum of item times {dur.sum():.0f} us; "
      f"empty {(L == 0).sum()} (mean {dur[L == 0].mean() if (L == 0).any() else 0:.1f} us), split slices {(nsl > 1).sum()}")
print("single-slice items by kept pairs: count | key init | raster | hash insert | record build | pixel pass | item (us, means)"
      " | share of the class's item time before stamp 2")
tot_before = tot_all = 0.0
for lo, hi in ((1, 64), (64, 128), (128, 256), (256, 512), (512, 1025), (1025, 1 << 30)):
    m = (L >= lo) & (L < hi) & (nsl == 1) & ~np.isnan(ras) & ~np.isnan(hsh) & ~np.isnan(rec)
    if not m.any():
        continue
    k0 = np.nan_to_num(keys[m], nan=0.0)
    a = [k0.mean(), (ras[m] - k0).mean(), (hsh[m] - ras[m]).mean(), (rec[m] - hsh[m]).mean(), (dur[m] - rec[m]).mean()]
    print(f"  [{lo:5d},{hi:6d}) {m.sum():5d} | " + " | ".join(f"{v:6.2f}" for v in a) + f" | {dur[m].mean():6.2f} | "
          f"{ras[m].sum() / dur[m].sum():.3f}")
    tot_before += ras[m].sum()
    tot_all += dur[m].sum()
sp = (nsl > 1)
if sp.any():
    print(f"  split slices: {sp.sum()} items, mean {dur[sp].mean():.2f} us, sum {dur[sp].sum():.0f} us (raster, slot write, "
          f"and on the last slice merge and shading)")
ne = L > 0
print(f"summed item time: all {dur.sum():.0f} us, non-empty {dur[ne].sum():.0f} us; single-slice items before stamp 2 "
      f"{tot_before:.0f} us = {tot_before / max(dur.sum(), 1e-9):.3f} of all item time "
      f"({tot_before / max(tot_all, 1e-9):.3f} of the single-slice items')")

# Items shaded from the key cache (k_keys_idx, k_keys_rec): stamp 2 once the item's first-round loads are issued, 4
# after the depth stores (KO_ALL), 5 past the barrier (the staged records are in LDS: loads waited for, records built
# or copied), 6 at the end of the pixel pass (the overflow loop follows).
ovf = ph[:, 5]
if not np.isnan(ovf).all():
    print("cached items by kept pairs: count | head (start -> loads issued) | records (-> in LDS, barrier) | pixel pass | "
          "overflow loop | item (us, means)")
    for lo, hi in ((1, 64), (64, 128), (128, 256), (256, 512), (512, 1025), (1025, 1 << 30)):
        m = (L >= lo) & (L < hi) & ~np.isnan(ras) & ~np.isnan(rec) & ~np.isnan(ovf)
        if not m.any():
            continue
        a = [ras[m].mean(), (rec[m] - ras[m]).mean(), (ovf[m] - rec[m]).mean(), (dur[m] - ovf[m]).mean()]
        print(f"  [{lo:5d},{hi:6d}) {m.sum():5d} | " + " | ".join(f"{v:6.2f}" for v in a) + f" | {dur[m].mean():6.2f}")
    first = t0.min()
    print(f"the 16 densest items against the kernel span ({span:.1f} us): kept pairs | start | head | records | pixel pass | "
          "overflow loop | item | end (us)")
    for i in np.argsort(-L, kind="stable")[:16]:
        print(f"  {L[i]:6d} | {t0[i] - first:6.2f} | {ras[i]:6.2f} | {rec[i] - ras[i]:6.2f} | {ovf[i] - rec[i]:6.2f} | "
              f"{dur[i] - ovf[i]:6.2f} | {dur[i]:6.2f} | {t0[i] - first + dur[i]:6.2f}")
    if hasattr(ctx, "key_record_batch_count"):
        print(f"key record batches {ctx.key_record_batch_count()}, totals {ctx.key_record_totals()}")
