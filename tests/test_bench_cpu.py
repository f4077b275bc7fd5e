"""bench.py's roofline bookkeeping (CPU): the frame fraction of an emulated
rank share uses that share's bytes, a real N-GPU line N x the peak, and PMC
traffic is reported only from a summary of the same configuration and share."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_frame_fraction_uses_the_owned_share_and_n_peaks():
    b = _bench()
    B = b.algorithmic_bytes(b.CONFIGS["c3"], 1_000_000)
    assert B == 425_126_400
    # round-2 emulated 8-way share: 0.0527 ms per frame for ~1/8 of the rows
    r = b.frame_roofline(B, 270 / 2160, 0.0527, 1)
    assert r["frame_frac"] < 1 and r["frame_algorithmic_bytes"] == int(B * 270 / 2160)
    # a real 8-GPU line at the same per-frame time moves the whole frame over 8 GPUs
    r8 = b.frame_roofline(B, 270 / 2160, 0.0527, 8)
    assert r8["frame_peak"] == 8 * b.PEAK_HBM_GBPS and r8["frame_frac"] < 1
    assert abs(r8["frame_frac"] - r["frame_frac"]) < 1e-3   # an eighth of the bytes per GPU either way


def test_pmc_traffic_only_for_the_same_config_and_share(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    (tmp_path / "profiles").mkdir()
    (tmp_path / "profiles" / "pmc_c3.json").write_text(json.dumps({"config": "c3", "hbm_bytes_per_launch": 7}))
    assert b.load_pmc_traffic("c3")[0] == 7
    assert b.load_pmc_traffic("c3", 8)[0] is None                  # a rank share: no unsharded counters
    assert b.load_pmc_traffic("c2")[0] is None
    assert b.load_pmc_traffic("c3", frame_out="yuv420p")[0] is None
    tag = "c3" + b.shard_tag(8, [6, 2, 2, 2, 2, 2, 2, 2])
    (tmp_path / "profiles" / f"pmc_{tag}.json").write_text(json.dumps({"config": tag, "hbm_bytes_per_launch": 5}))
    assert b.load_pmc_traffic("c3", 8, [6, 2, 2, 2, 2, 2, 2, 2])[0] == 5
    assert b.load_pmc_traffic("c3", 8)[0] is None


def test_committed_pmc_summaries_name_their_config():
    """Every profiles/pmc_*.json says which configuration and share it measured
    (the file name's tag), so bench.py never applies one config's counters to another."""
    pdir = os.path.join(ROOT, "profiles")
    for f in os.listdir(pdir):
        if f.startswith("pmc_") and f.endswith(".json"):
            d = json.load(open(os.path.join(pdir, f)))
            assert d["config"] == f[len("pmc_"):-len(".json")], f
            assert d["hbm_bytes_per_launch"] > 0


def test_plain_run_is_the_default_and_full_is_an_option():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = b.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


class _DumpCtx:
    """The readbacks dump_outputs takes from a context, of a seeded frame."""

    def __init__(self, W, H, shape):
        import numpy as np
        g = np.random.Generator(np.random.PCG64(7))
        self.shape = shape
        self.u8 = g.integers(0, 256, size=shape, dtype=np.uint8)
        self.f64 = g.uniform(0, 1, size=(H, W, 3))
        self.depth = g.integers(0, 2**32, size=(H, W), dtype=np.uint32)

    def frame_output_shape(self):
        return self.shape

    def get_frame_u8(self):
        return self.u8

    def get_buffer_numpy(self):
        return self.f64

    def get_depth_buffer(self):
        return self.depth


def test_dump_outputs_is_a_fixed_sample_within_64_mb(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 arrays, exact for the u8 frame and the
    u32 depth; a larger output is cut to the same seeded sample in every run;
    the caps keep all files of the largest case (RGB framebuffer: ipp = 4
    with alpha) under 64 MB."""
    import types
    import numpy as np
    b = _bench()
    assert b.DUMP_FRAME_ELEMS * 4 + b.DUMP_PIXELS * (4 + 1) * 8 + 3 * 128 <= 64 * 10**6
    W, H = 64, 48
    monkeypatch.setattr(b, "DUMP_FRAME_ELEMS", 5000)   # the planes (4608) whole, the RGB image (9216) sampled
    monkeypatch.setattr(b, "DUMP_PIXELS", 500)
    got = []
    for d, shape in (("a", (W * H * 3 // 2,)), ("b", (W * H * 3 // 2,)), ("rgb", (H, W, 3))):
        ctx = _DumpCtx(W, H, shape)
        run = types.SimpleNamespace(ctx=ctx, host=None, world=1, nsh=1, W=W, H=H)
        b.dump_outputs(run, 0, str(tmp_path / d))
        out = {f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))}
        assert sorted(out) == ["depth", "frame_output", "framebuffer"]
        assert out["frame_output"].dtype == np.float32 and out["framebuffer"].dtype == out["depth"].dtype == np.float64
        got.append((ctx, out))
    (ctx, a), (_, a2), (crgb, rgb) = got
    for k in a:
        assert np.array_equal(a[k], a2[k])                       # the same inputs, the same files
    assert np.array_equal(a["frame_output"], ctx.u8)
    px = b.dump_sample(W * H, 500, 2)
    assert a["framebuffer"].shape == (500, 3) and np.array_equal(a["framebuffer"], ctx.f64.reshape(-1, 3)[px])
    assert np.array_equal(a["depth"], ctx.depth.reshape(-1)[px].astype(np.float64))
    idx = b.dump_sample(W * H * 3, 5000, 1)
    assert rgb["frame_output"].shape == (5000,) and np.array_equal(rgb["frame_output"], crgb.u8.reshape(-1)[idx])
    assert len(set(idx.tolist())) == 5000 and np.all(np.diff(idx) > 0)
