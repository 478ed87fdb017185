// The register and LDS maps of the update tasks of the dataflow launch (dataflow.hip: df_syrk_tiles), in one place: which column of
// a wave's 32 an accumulator group or a column-operand fragment holds, where a lane's operand fragments lie in a slot of the operand
// ring, and how the LDS-DMA that fills the ring places a panel column.  The kernel computes its addresses with these functions and
// okkt_debug_dataflow_fragment (include/okkt.h) exports them, so tests/test_dataflow_fragments.py checks exactly what the kernel uses.
//
// A worker is 2 x 4 waves on a 128 x 128 tile: wave w owns rows 64 (w & 1) .. + 63 and columns 32 (w >> 1) .. + 31.  One k-step is
// 32 x v_mfma_f64_4x4x4 (four blocks of 4 x 4 x 4): the operands' k index is lane >> 4, the A (column) operand's index inside a
// block is lane & 3 and the same in all four blocks (lane >> 2) & 3, the B (row) operand's row is 2 (lane & 15) + (rb & 1) + 32 (rb >> 1),
// and an accumulator holds the column that lanes with (lane & 3) == its (lane >> 4) multiplied with.
//
// map 0 (the earlier one, -DOKKT_DF_CONTIG=0): fragment cg of a lane is column 4 cg + (lane & 3) -- a lane's eight fragments lie 4 doubles apart, the
//   compiler fetches them as 4 x ds_read2_b64 (8 LDS-array cycles each); both operand images have leading dimension kSyrkLd = 144.
// map 1: fragment cg of a lane is column 8 (lane & 3) + cg -- 64 contiguous bytes, 4 x ds_read_b128 (4 cycles each).  Only the names
//   of a wave's columns change: every entry still receives its products in ascending k, the factor is bitwise the same.
//
// Banks (ds_read_b128: bank (a / 4) mod 64, lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): a group holds
// lanes of two neighbouring k (lane >> 4 = 0 and 1, or 2 and 3), i.e. of two neighbouring panel columns.
//   row fragments: the 8 lanes of one k cover dwords 16 .. 47 of a 64-dword window and the 8 of the other 0 .. 15 and 48 .. 63 -- disjoint
//     exactly when the two panel columns are a multiple of 64 dwords apart.  ld = 144 puts them 32 apart: 2-way.  ld = 128: none.
//   column fragments (map 1): the four distinct addresses of one k are dwords 16 i + 4 j .. + 3 (i = lane & 3, read j of four); the
//     other k's must fall between them: panel columns 4, 8 or 12 (mod 16) dwords apart.  ld = 130: k = 0 .. 3 at +0, +4, +8, +12.
// The two conditions exclude each other for one leading dimension, and the W and L images are filled by separate DMA instructions:
// each image gets its own (128 and 130 doubles), every read of both kinds is conflict-free, and no rotation of a panel column's rows
// is needed (df_ring_rot is 0; the DMA's source address is lane-linear).  A slot is KC (128 + 130) doubles: 129 KiB for 2 x 32 columns.
#pragma once

#if defined(__HIPCC__)
#define OKKT_FRAG_HD __host__ __device__
#else
#define OKKT_FRAG_HD
#endif

namespace okkt {

constexpr int kDfFragLdOld = 144;   // = kSyrkLd (front_device.h; dataflow.hip asserts it)

// leading dimensions (doubles) of the W (row operand) and L (column operand) images of a ring slot
OKKT_FRAG_HD constexpr int df_ring_ld_w(int map) { return map ? 128 : kDfFragLdOld; }
OKKT_FRAG_HD constexpr int df_ring_ld_l(int map) { return map ? 130 : kDfFragLdOld; }
OKKT_FRAG_HD constexpr int df_ring_slot_doubles(int map, int kc) { return kc * (df_ring_ld_w(map) + df_ring_ld_l(map)); }
// rows by which the DMA rotates panel column p inside its image column: none in either map (see above)
OKKT_FRAG_HD constexpr int df_ring_rot(int map, int p) { return 0 * (map + p); }

// column (inside the wave's 32) of accumulator group cg / of column-operand fragment cg in a lane
OKKT_FRAG_HD constexpr int df_frag_acc_col(int map, int lane, int cg) { return map ? 8 * (lane >> 4) + cg : 4 * cg + (lane >> 4); }
OKKT_FRAG_HD constexpr int df_frag_a_col(int map, int lane, int cg) { return map ? 8 * (lane & 3) + cg : 4 * cg + (lane & 3); }

// offsets (doubles, from the slot's first) of a lane's operand fragments of k-step kk of a chunk of kc panel columns:
// column fragment cg (0 .. 7) and row fragment rb (0 .. 3)
OKKT_FRAG_HD constexpr int df_frag_a_off(int map, int kc, int wave, int lane, int kk, int cg) {
  return kc * df_ring_ld_w(map) + (4 * kk + (lane >> 4)) * df_ring_ld_l(map) + 32 * (wave >> 1) + df_frag_a_col(map, lane, cg);
}
OKKT_FRAG_HD constexpr int df_frag_b_off(int map, int wave, int lane, int kk, int rb) {
  return (4 * kk + (lane >> 4)) * df_ring_ld_w(map) + 64 * (wave & 1) + 2 * (lane & 15) + (rb & 1) + 32 * (rb >> 1);
}

}  // namespace okkt
