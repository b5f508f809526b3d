"""CPU-only checks of the symmetric 16-bit scan's schedule (mmf_debug_symmetric_schedule, DESIGN.md §4.1 "Symmetric scan"):
the two launches' work tables cover every ordered (row block, column tile) pair exactly once — as a plain pair of launch 0, as
a pair launch 1 scans directly, or as the mirror image of one — for every row-block count and super-block size."""
import ctypes

import numpy as np
import pytest

TILES_PER_BLOCK = 8          # a row block is 256 rows, a column tile 32
TILE_BYTES = 32 * 512 * 2    # a tile of the padded-dim-512 operand image


def tables(nb, G):
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    out = []
    for launch in (0, 1):
        grid = L.mmf_debug_symmetric_schedule(nb, G, launch, None, 0)
        assert grid > 0 and grid % 8 == 0
        t = np.zeros((grid, 8), dtype=np.int32)
        assert L.mmf_debug_symmetric_schedule(nb, G, launch, ctypes.c_void_p(t.ctypes.data), grid) == grid
        out.append(t)
    return out


def ranges(e):
    return [(int(e[1]), int(e[2])), (int(e[3]), int(e[4]))]


@pytest.mark.parametrize("G", [1, 2, 3, 8, 32])
def test_every_ordered_pair_is_covered_exactly_once(G):
    for nb in range(1, 81):
        ta, tb = tables(nb, G)
        tiles = nb * TILES_PER_BLOCK
        cover = np.zeros((nb, tiles), dtype=np.int32)
        cols = np.zeros(nb, dtype=np.int64)
        for launch, t in enumerate((ta, tb)):
            seen = set()
            for e in t:
                rb = int(e[0])
                if rb < 0:
                    continue
                assert 0 <= rb < nb and rb not in seen, "one workgroup per row block and launch"
                seen.add(rb)
                for b, c in ranges(e):
                    assert c >= 0 and c % TILES_PER_BLOCK == 0 and 0 <= b and b + c <= tiles
                    assert (b + c) * TILE_BYTES < 2 ** 32, "a workgroup's range stays inside the 32-bit DMA offset"
                    cover[rb, b:b + c] += 1                                # plain, or scanned directly
                    cols[rb] += c
                    if launch == 1:                                        # ... and its mirror image: the tiles of the row
                        for cb in range(b // TILES_PER_BLOCK, (b + c) // TILES_PER_BLOCK):   # block, for the rows of these tiles
                            cover[cb, rb * TILES_PER_BLOCK:(rb + 1) * TILES_PER_BLOCK] += 1
                first = ranges(e)[0]
                assert first[1] > 0 or ranges(e)[1][1] == 0, "the first range is the non-empty one"
            assert len(seen) == nb or (launch == 1 and len(seen) in (0, nb)), (nb, G, launch)
        assert (cover == 1).all(), (nb, G)
        assert cols.max() - cols.min() <= G * TILES_PER_BLOCK, "columns per row block differ by at most one super-block"


def super_block_of(rb, nb, G):
    ns = max(1, nb // G)
    return min(rb // G, ns - 1)          # the left-over row blocks belong to the last super-block


def test_blocks_of_a_super_block_share_an_xcd_and_a_stretch_of_block_ids():
    for nb, G in ((1024, 32), (80, 8), (37, 3), (514, 32)):
        ns = max(1, nb // G)
        for t in tables(nb, G):
            for b, e in enumerate(t):
                if e[0] >= 0:
                    sb = super_block_of(int(e[0]), nb, G)
                    assert sb % 8 == b % 8
                    if int(e[0]) < ns * G:
                        assert sb // 8 == b // (8 * G)
                    else:                                     # left-over row blocks: a stretch of their own behind the others
                        assert b // (8 * G) == (ns + 7) // 8


def test_no_super_block_is_short():
    """Launch 0 gives a row its threshold from the columns of its own super-block: every row block must see at least G row blocks
    there (a short last super-block would leave its rows with thresholds from a handful of columns)."""
    for G in (1, 2, 3, 8, 32):
        for nb in range(G, 200):
            ta, _ = tables(nb, G)
            for e in ta:
                if e[0] >= 0:
                    own = [c for b, c in ranges(e) if b <= int(e[0]) * TILES_PER_BLOCK < b + c]
                    assert len(own) == 1 and G * TILES_PER_BLOCK <= own[0] < 2 * G * TILES_PER_BLOCK, (nb, G)


def test_one_super_block_is_todays_scan():
    ta, tb = tables(20, 32)
    assert (tb[:, 0] < 0).all()
    live = ta[ta[:, 0] >= 0]
    assert sorted(live[:, 0]) == list(range(20))
    assert (live[:, 1] == 0).all() and (live[:, 2] == 160).all() and (live[:, 4] == 0).all()


def test_bad_arguments_are_rejected():
    import multimodal_fusion_amd as mmf
    L = mmf._lib.lib()
    assert L.mmf_debug_symmetric_schedule(0, 32, 0, None, 0) < 0
    assert L.mmf_debug_symmetric_schedule(8, 0, 0, None, 0) < 0
    assert L.mmf_debug_symmetric_schedule(8, 2, 2, None, 0) < 0
    t = np.zeros((4, 8), dtype=np.int32)
    assert L.mmf_debug_symmetric_schedule(64, 2, 0, ctypes.c_void_p(t.ctypes.data), 4) < 0
