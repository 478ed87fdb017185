"""The register and LDS maps of the update tasks of the dataflow launch (csrc/df_fragments.h, used by df_syrk_tiles in
csrc/dataflow.hip), checked on the CPU through okkt_debug_dataflow_fragment -- the functions the kernel itself computes its
addresses with.  map 1 is the contiguous map (a lane's eight column fragments are eight neighbouring columns, the operand ring
has its own two images), map 0 the earlier one (fragments four columns apart, both images with leading dimension 144).

The bank model is this file's own transcription of the LDS table of the MI355X guide: ds_read_b128 is served in four groups of
sixteen lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, one LDS cycle per group; the bank of byte address a
is (a / 4) mod 64; lanes of a group with the same address share one access, every further distinct address on a bank costs the
group one more cycle."""
import itertools

import numpy as np
import pytest

from onephase_jl_amd import _lib

NEW, OLD = 1, 0
B128_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


@pytest.fixture(scope="module")
def frag():
    f = _lib.load().okkt_debug_dataflow_fragment

    def call(*a):
        v = f(*a)
        assert v >= 0, a
        return int(v)
    return call


def geometry(frag, m):
    return dict(zip(("ldw", "ldl", "slot", "kc", "stages", "built", "lds", "ld_steps"), (frag(m, 5, 0, 0, 0, i) for i in range(8))))


def extra_cycles_b128(byte_addr):
    """Extra LDS cycles (beyond the four of a conflict-free instruction) of one ds_read_b128 with the 64 lanes' byte addresses."""
    extra = 0
    for g in B128_GROUPS:
        per_bank = {}
        for a in {byte_addr[l] for l in g}:
            assert a % 16 == 0
            for dw in range(a // 4, a // 4 + 4):
                per_bank.setdefault(dw % 64, set()).add(dw)
        extra += max(len(v) for v in per_bank.values()) - 1
    return extra


def test_the_lane_groups_cover_the_wave_once():
    assert sorted(itertools.chain(*B128_GROUPS)) == list(range(64)) and all(len(g) == 16 for g in B128_GROUPS)


@pytest.mark.parametrize("m", [NEW, OLD])
def test_every_entry_of_the_tile_has_one_owner(frag, m):
    """8 waves x 64 lanes x 8 accumulator groups x 4 row slots = 128 x 128: row from the lane's row fragment (lane & 15 and the slot),
    column from the accumulator group (lane >> 4), as v_mfma_f64_4x4x4 delivers its blocks."""
    g = geometry(frag, m)
    owners = np.zeros((128, 128), dtype=np.int64)
    for w in range(8):
        for lane in range(64):
            rows = [frag(m, 3, w, lane, 0, rb) - (lane >> 4) * g["ldw"] for rb in range(4)]
            cols = [32 * (w >> 1) + frag(m, 0, w, lane, 0, cg) for cg in range(8)]
            assert all(64 * (w & 1) <= r < 64 * (w & 1) + 64 for r in rows)
            for r in rows:
                for c in cols:
                    owners[r, c] += 1
    assert (owners == 1).all()


@pytest.mark.parametrize("m", [NEW, OLD])
def test_an_accumulator_holds_the_column_its_operand_brought(frag, m):
    """The accumulator of a lane with lane >> 4 = i collects the products of the A fragments of the lanes with lane & 3 = i."""
    for lane_a in range(64):
        for lane_c in range(64):
            if lane_c >> 4 == lane_a & 3:
                for cg in range(8):
                    assert frag(m, 1, 0, lane_a, 0, cg) == frag(m, 0, 0, lane_c, 0, cg)
    # the A operand is a broadcast: the same in the four blocks of an MFMA
    for lane in range(64):
        assert [frag(m, 1, 0, lane, 0, cg) for cg in range(8)] == [frag(m, 1, 0, lane & ~12, 0, cg) for cg in range(8)]


@pytest.mark.parametrize("m", [NEW, OLD])
def test_the_fragments_read_what_the_dma_wrote(frag, m):
    """The LDS-DMA puts row x of panel column p of the W image at p ldw + (x + rot) mod 128, of the L image behind the kc W
    columns at p ldl + (x + rot) mod 128; a fragment of k-step kk in a lane belongs to panel column 4 kk + (lane >> 4)."""
    g = geometry(frag, m)
    assert g["slot"] == g["kc"] * (g["ldw"] + g["ldl"]) and min(g["ldw"], g["ldl"]) >= 128
    assert g["stages"] * g["slot"] * 8 <= g["lds"] <= 160 * 1024
    assert g["ld_steps"] == 144 and (m == NEW or g["ldw"] == g["ldl"] == 144)
    for w, lane, kk in itertools.product(range(8), range(64), range(g["kc"] // 4)):
        p = 4 * kk + (lane >> 4)
        rot = frag(m, 4, w, lane, kk, 0)
        assert rot % 2 == 0      # the DMA moves 16 bytes per lane
        for cg in range(8):
            col = 32 * (w >> 1) + frag(m, 1, w, lane, kk, cg)
            assert frag(m, 2, w, lane, kk, cg) == g["kc"] * g["ldw"] + p * g["ldl"] + (col + rot) % 128
        for rb in range(4):
            row = 64 * (w & 1) + 2 * (lane & 15) + (rb & 1) + 32 * (rb >> 1)
            assert frag(m, 3, w, lane, kk, rb) == p * g["ldw"] + (row + rot) % 128


def test_a_lanes_column_fragments_are_64_contiguous_aligned_bytes(frag):
    g = geometry(frag, NEW)
    for w, lane, kk in itertools.product(range(8), range(64), range(g["kc"] // 4)):
        off = [frag(NEW, 2, w, lane, kk, cg) for cg in range(8)]
        assert off == list(range(off[0], off[0] + 8)) and (8 * off[0]) % 16 == 0
        # ... and inside one image column, so the rotation (checked above) cannot have split them
        assert (off[0] - g["kc"] * g["ldw"]) % g["ldl"] + 8 <= 128
    # the earlier map: four doubles apart (what the compiler could only fetch with ds_read2_b64)
    assert [frag(OLD, 2, 0, 5, 0, cg) - frag(OLD, 2, 0, 5, 0, 0) for cg in range(8)] == [4 * cg for cg in range(8)]


def reads_of_a_chunk(frag, m, slot_byte0):
    """(kind, wave, k-step, index, the 64 byte addresses) of every 16-byte operand read of a chunk as map 1 issues them: two row
    reads (slots 0 - 1 and 2 - 3) and four column reads per k-step."""
    g = geometry(frag, m)
    for w, kk in itertools.product(range(8), range(g["kc"] // 4)):
        for h in range(2):
            yield "row", w, kk, h, [slot_byte0 + 8 * frag(m, 3, w, lane, kk, 2 * h) for lane in range(64)]
        for j in range(4):
            yield "col", w, kk, j, [slot_byte0 + 8 * frag(m, 2, w, lane, kk, 2 * j) for lane in range(64)]


def test_the_rings_image_is_conflict_free_for_both_operand_reads(frag):
    g = geometry(frag, NEW)
    n = 0
    for s in range(g["stages"]):
        for kind, w, kk, j, addr in reads_of_a_chunk(frag, NEW, s * g["slot"] * 8):
            assert extra_cycles_b128(addr) == 0, (s, kind, w, kk, j)
            n += 1
    assert n == g["stages"] * 8 * (g["kc"] // 4) * 6


def test_the_earlier_image_has_two_way_conflicts_on_the_row_reads(frag):
    """Leading dimension 144: neighbouring panel columns lie 288 = 32 (mod 64) dwords apart, the eight lanes of the second k of a
    lane group fall on the banks of the first: every group of every row read takes two cycles instead of one."""
    for kind, w, kk, j, addr in reads_of_a_chunk(frag, OLD, 0):
        if kind == "row":
            assert extra_cycles_b128(addr) == 4, (w, kk, j)
    # and neither leading dimension of the new ring would serve the other operand
    g = geometry(frag, NEW)
    lane_l4 = np.arange(64) >> 4
    row_at_ldl = [8 * (int(l4) * g["ldl"] + 2 * (lane & 15)) for lane, l4 in enumerate(lane_l4)]
    col_at_ldw = [8 * (int(l4) * g["ldw"] + 8 * (lane & 3)) for lane, l4 in enumerate(lane_l4)]
    assert extra_cycles_b128(row_at_ldl) > 0 and extra_cycles_b128(col_at_ldw) > 0


def test_bad_arguments_are_refused():
    f = _lib.load().okkt_debug_dataflow_fragment
    for a in [(2, 0, 0, 0, 0, 0), (1, 0, 8, 0, 0, 0), (1, 0, 0, 64, 0, 0), (1, 2, 0, 0, 8, 0), (1, 0, 0, 0, 0, 8), (1, 3, 0, 0, 0, 4), (1, 6, 0, 0, 0, 0)]:
        assert f(*a) < 0
