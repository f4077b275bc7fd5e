"""The numpy restatement of the key records' totals (tests/key_records_ref.py)
on its own, and the properties of the GPU tests' fixtures
(tests/test_key_records_gpu.py): SMALL's store fits under the cap, whole or
sharded; BIG's holds records past KI_RT in most tiles and fits only as a
shard's -- unsharded it is 10.5 MB against a 6.1 MB framebuffer, so that
generation stays on the key index; and the pixel-triangle mesh of the no-memory
case exceeds the cap on a frame small enough for a quick test."""
import numpy as np
import pytest

import key_index_ref as I
import key_records_ref as KR
import scenes

W, H = 640, 400
SMALL, BIG = (60, 200), (250, 700)
OVER = (64, 32)                                  # the frame of the pixel-triangle mesh


def test_hand_made_tiles():
    """key_index_ref's hand-made frame: three winners in the left tile, one in
    the right; 3 appears in one tile only, so four records."""
    ids = np.zeros((20, 100), dtype=np.int64)
    ids[0, 5:9] = 7
    ids[0, 9] = 3
    ids[1, 0:3] = 3
    ids[2, 0:6] = 9
    ids[4, 64:100] = 5
    assert KR.records(ids, (100, 20)) == 4
    assert KR.totals(ids, (100, 20), 2) == {"slots": 2, "records": 4, "bytes": 512}
    # a winner that spans both tiles has a record in each
    ids[4, 60:64] = 5
    assert KR.records(ids, (100, 20)) == 5


def test_the_cap_is_the_f64_framebuffer():
    assert KR.cap_bytes((640, 400)) == 640 * 400 * 24 and KR.cap_bytes((640, 400), True) == 640 * 400 * 32
    n = KR.cap_bytes((64, 32)) // KR.REC_BYTES   # 384 records fill 64 x 32 x 24 bytes exactly
    assert n * KR.REC_BYTES == KR.cap_bytes((64, 32))
    assert KR.fits(n, (64, 32)) and not KR.fits(n + 1, (64, 32))
    ids = np.arange(1, 64 * 32 + 1, dtype=np.int64).reshape(32, 64)   # every pixel its own winner
    assert KR.records(ids, (64, 32)) == 2048 and KR.totals(ids, (64, 32), 1) is None


@pytest.mark.parametrize("mesh", [SMALL, BIG])
def test_which_sphere_stores_fit(oracle, mesh):
    xy, z, _ = scenes.sphere_mesh(W, H, *mesh)
    ids = I.winner_ids(xy, z, (W, H))
    distinct, _ = I.tile_index(ids, (W, H))
    n = KR.records(ids, (W, H))
    assert n == distinct.sum() == (82051 if mesh == BIG else 9408)
    assert KR.fits(n, (W, H)) == (mesh == SMALL)
    assert (n > np.minimum(distinct, I.KI_RT).sum()) == (mesh == BIG)   # BIG: records past the staged ones
    for shard in [(2, 1), (8, 3)]:
        rows = distinct.reshape(-1, (W + I.TW - 1) // I.TW)
        part = KR.records(ids, (W, H), shard)
        assert part == rows[np.arange(len(rows)) % shard[0] == shard[1]].sum() > 0
        assert KR.fits(part, (W, H))             # (the cap is the whole context's framebuffer, sharded or not)


def test_the_pixel_triangles_exceed_the_cap(oracle):
    xy, z, _ = KR.pixel_triangles(OVER)
    ids = I.winner_ids(xy, z, OVER)
    assert len(np.unique(ids[ids > 0])) == OVER[0] * OVER[1]          # every triangle wins exactly its pixel
    assert KR.records(ids, OVER) == 2048
    assert 2048 * KR.REC_BYTES > KR.cap_bytes(OVER)
    assert KR.scene_totals(xy, z, OVER) is None
