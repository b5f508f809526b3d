"""CPU-only checks of the symmetric 16-bit scan's schedule with its two switches (mmf_debug_symmetric_schedule, DESIGN.md §4.1
"Two phases" and "Antipodal pairs once"): MMF_SYMMETRIC_PHASES = 1 / 2 (the single cyclic look-back / the wrap-around pairs in a
second phase behind all others) x MMF_SYMMETRIC_ANTIPODAL = 0 / 1 (the antipodal super-block pair in launch 0 from both sides /
once, symmetric, as the later super-block's last range).  mmf_debug_symmetric_schedule shows the two-phase table only when
MMF_SYMMETRIC_PHASES=2 is set (a scan takes it when the variable is unset too); words 5 and 6 of an entry are its list slot and
its phase (0: a table without phases, 1 / 2: phase A / B).

The ordering property, as it can hold with a super-block's row blocks on one XCD's ids of a stretch of 8 G block ids: a PHASE-B
entry comes behind every phase-A entry of the table, so behind all those of its candidates; a PHASE-A entry scans super-blocks
below its own, whose phase-A entries lie in an earlier stretch or — eight super-blocks interleave their ids there — in its own."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

TILES_PER_BLOCK = 8          # a row block is 256 rows, a column tile 32
TILE_BYTES = 32 * 512 * 2    # a tile of the padded-dim-512 operand image
KEYS = ("MMF_SYMMETRIC_PHASES", "MMF_SYMMETRIC_ANTIPODAL", "MMF_SYMMETRIC_LIVE")
SWITCHES = [(1, 0), (1, 1), (2, 0), (2, 1)]


@contextlib.contextmanager
def switches(phases, antipodal, live=None):
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ["MMF_SYMMETRIC_PHASES"] = str(phases)
    os.environ["MMF_SYMMETRIC_ANTIPODAL"] = str(antipodal)
    if live is not None:
        os.environ["MMF_SYMMETRIC_LIVE"] = str(live)
    try:
        yield
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


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


def super_block_of(rb, nb, G):
    ns = max(1, nb // G)
    return min(rb // G, ns - 1)          # the left-over row blocks belong to the last super-block


def candidate_super_blocks(e, nb, G):
    return {super_block_of(t // TILES_PER_BLOCK, nb, G) for b, c in ranges(e) for t in range(b, b + c, TILES_PER_BLOCK)}


@pytest.mark.parametrize("phases,antipodal", SWITCHES)
@pytest.mark.parametrize("G", [1, 2, 3, 8, 32])
def test_schedule(G, phases, antipodal):
    with switches(phases, antipodal):
        for nb in range(1, 81):
            check(nb, G, phases, antipodal)


def check(nb, G, phases, antipodal):
    ta, tb = tables(nb, G)
    ns = max(1, nb // G)
    tiles = nb * TILES_PER_BLOCK
    per = 8 * G
    where = (nb, G, phases, antipodal)
    # ---- every ordered (row, column) pair exactly once; ranges are multiples of 8 tiles --------------------------------------
    cover = np.zeros((nb, tiles), dtype=np.int32)
    for launch, t in enumerate((ta, tb)):
        for e in t:
            rb = int(e[0])
            if rb < 0:
                continue
            assert 0 <= rb < nb
            for b, c in ranges(e):
                assert c >= 0 and c % TILES_PER_BLOCK == 0 and b % TILES_PER_BLOCK == 0 and 0 <= b and b + c <= tiles, where
                assert (b + c) * TILE_BYTES < 2 ** 32
                cover[rb, b:b + c] += 1
                if launch == 1:                      # a symmetric range serves the mirror image too
                    for cb in range(b // TILES_PER_BLOCK, (b + c) // TILES_PER_BLOCK):
                        cover[cb, rb * TILES_PER_BLOCK:(rb + 1) * TILES_PER_BLOCK] += 1
            assert ranges(e)[0][1] > 0, "an entry with a row block has work, and its first range is the non-empty one"
    assert (cover == 1).all(), where
    # ---- launch 0: one entry per row block, slot 0, no phase; no super-block is short ------------------------------------------
    live0 = ta[ta[:, 0] >= 0]
    assert sorted(live0[:, 0]) == list(range(nb)) and (live0[:, 5] == 0).all() and (live0[:, 6] == 0).all(), where
    for e in live0:
        own = [c for b, c in ranges(e) if b <= int(e[0]) * TILES_PER_BLOCK < b + c]
        if nb >= G:
            assert len(own) == 1 and G * TILES_PER_BLOCK <= own[0] < 2 * G * TILES_PER_BLOCK, where
        if antipodal and ns % 2 == 0 and ns >= 4:
            assert int(e[4]) == 0, "launch 0 scans the own super-block alone"
        elif ns % 2 == 0 and ns >= 2:
            assert int(e[4]) > 0, "launch 0 scans the antipodal super-block too (two super-blocks: always)"
    # ---- the symmetric launch: at most one entry per row block and phase, distinct list slots -----------------------------------
    seen = {}
    for b, e in enumerate(tb):
        if e[0] < 0:
            continue
        rb, slot, phase = int(e[0]), int(e[5]), int(e[6])
        assert phase in ((1, 2) if phases == 2 else (0,)) and slot in (0, 1), where
        assert (rb, phase) not in seen, "one entry per row block and phase"
        seen[(rb, phase)] = slot
        assert slot == (1 if phase == 2 else 0)
        # a super-block's row blocks take one XCD's ids of one stretch, within each phase
        sb = super_block_of(rb, nb, G)
        assert sb % 8 == b % 8, where
    by_rb = {}
    for (rb, phase), slot in seen.items():
        by_rb.setdefault(rb, []).append(slot)
    assert all(len(s) == len(set(s)) for s in by_rb.values())
    # ---- ordering ------------------------------------------------------------------------------------------------------------
    if phases == 2:
        ids_a = {}                                   # super-block -> block ids of its phase-A entries
        for b, e in enumerate(tb):
            if e[0] >= 0 and e[6] == 1:
                ids_a.setdefault(super_block_of(int(e[0]), nb, G), []).append(b)
        last_a = max((max(v) for v in ids_a.values()), default=-1)
        lengths_b = []
        for b, e in enumerate(tb):
            if e[0] < 0:
                continue
            sb = super_block_of(int(e[0]), nb, G)
            cands = candidate_super_blocks(e, nb, G)
            assert sb not in cands
            if e[6] == 2:
                assert b > last_a, "phase B runs behind all of phase A"
                assert int(e[4]) == 0 and int(e[1]) + int(e[2]) == tiles, "what the look-back lost: one range up to the last tile"
                lengths_b.append((b // per, int(e[2])))
            else:
                for c in cands:
                    assert c < sb, "phase A never wraps"
                    # the candidate's phase-A entries (if it has work there): an earlier stretch of ids, or the scanner's own
                    assert all(i // per <= b // per for i in ids_a.get(c, [])), where
                    if c // 8 < sb // 8 and int(e[0]) < ns * G:
                        assert all(i < b for i in ids_a.get(c, [])), where
        # longest first: a later stretch of phase B holds no longer range than an earlier one
        for (s0, n0) in lengths_b:
            for (s1, n1) in lengths_b:
                assert not (s1 > s0 and n1 > n0), where
    # ---- antipodal pairs once: the later super-block scans the earlier one as its last range -------------------------------------
    if antipodal and ns % 2 == 0 and ns >= 4:
        for e in tb:
            if e[0] < 0 or e[6] == 2:
                continue
            sb = super_block_of(int(e[0]), nb, G)
            if sb >= ns // 2:
                last = ranges(e)[1] if e[4] > 0 else ranges(e)[0]
                assert last[0] == (sb - ns // 2) * G * TILES_PER_BLOCK and last[1] == G * TILES_PER_BLOCK, where


def test_the_look_ahead_tables_stay_as_they_were():
    """MMF_SYMMETRIC_LIVE = 0 / 2 (the A/B arms that look ahead) take neither switch."""
    for live in (0, 2):
        for nb, G in ((7, 1), (37, 3), (64, 8), (80, 2)):
            with switches(1, 0, live):
                old = tables(nb, G)
            with switches(2, 1, live):
                new = tables(nb, G)
            assert all(np.array_equal(a, b) for a, b in zip(old, new))


def test_unset_switch_shows_the_single_phase_table():
    old = {k: os.environ.pop(k, None) for k in KEYS}
    try:
        default = tables(40, 2)
    finally:
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v
    with switches(1, 0):
        single = tables(40, 2)
    assert all(np.array_equal(a, b) for a, b in zip(default, single))
    assert (default[1][:, 6] == 0).all()


def test_the_bench_shape():
    """1024 row blocks, G = 32: 32 super-blocks, h = 15.  Phase A: super-block b scans min(b, 15) super-blocks; phase B: b < 15
    scans 15 - b; 1024 + 512 + 8 block ids."""
    with switches(2, 0):
        _, tb = tables(1024, 32)
    assert len(tb) == 1544
    for e in tb:
        if e[0] < 0:
            continue
        sb = int(e[0]) // 32
        want = min(sb, 15) if e[6] == 1 else 15 - sb
        assert int(e[2]) + int(e[4]) == want * 32 * TILES_PER_BLOCK and want > 0
    assert (tb[:, 0] >= 0).sum() == 31 * 32 + 15 * 32
