"""The numpy restatement of the key index's totals (tests/key_index_ref.py) on
its own, and the properties of the GPU test's fixtures
(tests/test_key_index_gpu.py) that decide which path a tile takes: SMALL never
exceeds the KI_RT staged winners of a tile, BIG does in most tiles -- so the GPU
tests cannot silently miss the staged-only or the direct path."""
import numpy as np
import pytest

import key_cache_ref as K
import key_index_ref as I
import scenes

W, H = 640, 400
SMALL, BIG = (60, 200), (250, 700)
_IDS = {}


def _ids(mesh):
    if mesh not in _IDS:
        xy, z, _ = scenes.sphere_mesh(W, H, *mesh)
        _IDS[mesh] = (xy, z, I.winner_ids(xy, z, (W, H)))
    return _IDS[mesh]


def test_small_never_goes_direct(oracle):
    xy, z, ids = _ids(SMALL)
    distinct, direct = I.tile_index(ids, (W, H))
    assert (distinct > 0).sum() == 78 and distinct.max() == 243 <= I.KI_RT
    assert direct.sum() == 0
    t = I.totals(ids, (W, H), K.scene_totals(xy, z, (W, H))[0]["tiles"])
    assert t["staged"] == distinct.sum() and t["direct"] == 0
    assert t["tiles"] >= 78 and t["bytes"] == t["tiles"] * I.SLOT_BYTES


def test_big_goes_direct_heavily(oracle):
    xy, z, ids = _ids(BIG)
    distinct, direct = I.tile_index(ids, (W, H))
    assert (distinct > 0).sum() == 78 and (distinct > I.KI_RT).sum() == 68 and distinct.max() == 1715
    assert ((direct > 0) == (distinct > I.KI_RT)).all()
    t = I.totals(ids, (W, H), 78)
    assert t["staged"] == np.minimum(distinct, I.KI_RT).sum() < distinct.sum()
    # every winner past the staged ones has a pixel, and a tile has TH * TW of them
    assert (direct >= distinct - np.minimum(distinct, I.KI_RT)).all()
    assert (direct <= I.TH * I.TW - I.KI_RT)[distinct > I.KI_RT].all()


@pytest.mark.parametrize("shard", [(2, 1), (8, 3)])
def test_shards_sum_over_their_tile_rows(oracle, shard):
    _, _, ids = _ids(SMALL)
    distinct, _ = I.tile_index(ids, (W, H))
    rows = distinct.reshape(-1, (W + I.TW - 1) // I.TW)
    want = rows[np.arange(len(rows)) % shard[0] == shard[1]].sum()
    assert I.totals(ids, (W, H), 0, shard)["staged"] == want > 0


def test_hand_made_tiles():
    """Two tiles of a 100 x 20 frame: three winners left, of which the one seen
    last is unstaged under rt = 2; the right tile is cut by the frame edge."""
    ids = np.zeros((20, 100), dtype=np.int64)
    ids[0, 5:9] = 7
    ids[0, 9] = 3
    ids[1, 0:3] = 3
    ids[2, 0:6] = 9
    ids[4, 64:100] = 5
    distinct, direct = I.tile_index(ids, (100, 20), rt=2)
    assert list(distinct) == [3, 1] and list(direct) == [6, 0]
    assert I.totals(ids, (100, 20), 2, rt=2) == {"tiles": 2, "staged": 3, "direct": 6, "bytes": 2 * I.SLOT_BYTES}
    assert I.totals(ids, (100, 20), 2) == {"tiles": 2, "staged": 4, "direct": 0, "bytes": 2 * I.SLOT_BYTES}
