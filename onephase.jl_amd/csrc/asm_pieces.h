// Flat work records of the big-front assembly (numeric.hip: k_big_assemble_staged): for every unit = (front
// column, row chunk) of a big front the contiguous run of the pieces that land in it, and the column's A entries of that chunk.
// A piece is the part of one extend-add item (a child's contribution-block column) whose parent rows fall into the chunk; pieces that
// are empty in a chunk are not emitted.  Within a unit the pieces keep the order of the items (children ascending): the summation
// order of the assembly is the order of the list.  Built once per plan on the host; plain C++, run under the sanitizers by
// asan_driver.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "symbolic.h"

namespace okkt {

// rows [0, n) of the piece: value i sits at arena[src + i], its row in the parent front is rel[rel_pos + i]
struct alignas(16) AsmPiece { int64_t src; int rel; int n; };
static_assert(sizeof(AsmPiece) == 16, "one 16-byte load per piece and lane");
// unit (pc, t) of front s is units[unit_base[s] + t * f + pc]: its pieces, and the A entries (aent_src / aent_dst positions) of
// column pc whose rows lie in chunk t
struct alignas(32) AsmUnit { int64_t piece0; int64_t a0; int np; int na; int pad[2]; };
static_assert(sizeof(AsmUnit) == 32, "host and device agree on the record");

struct AsmPlan {
  std::vector<int64_t> unit_base;   // [nsuper] first unit of a big front, -1 otherwise
  std::vector<AsmUnit> units;
  std::vector<AsmPiece> pieces;
  int64_t items = 0;                // extend-add items covered (child column, whole)
  int64_t bytes() const { return (int64_t)(unit_base.size() * sizeof(int64_t) + units.size() * sizeof(AsmUnit) + pieces.size() * sizeof(AsmPiece)); }
};

// big[s] != 0: front s is assembled by the big-front kernels.  cb_base[c]: arena offset of entry (0, 0) of child c's contribution
// block (leading dimension f_c); read only for children of big fronts.  chunk: rows per chunk.  Returns "" or an error message.
inline std::string asm_build_pieces(const Symbolic& S, const std::vector<char>& big, const std::vector<int64_t>& cb_base, int chunk, AsmPlan& A) {
  A = AsmPlan();
  const int ns = S.nsuper;
  if ((int)big.size() < ns || (int)cb_base.size() < ns || chunk <= 0) return "assembly records: the inputs do not cover the supernodes";
  if (S.rel.size() > (size_t)INT32_MAX) return "assembly records: the rel lists pass 2^31 entries";
  A.unit_base.assign(ns, -1);
  // inverted lists: per column of a big front the items (child, jj) that land on it, children ascending
  std::vector<int64_t> col_base(ns, -1);
  int64_t ncols = 0, nunits = 0;
  for (int s = 0; s < ns; ++s)
    if (big[s]) {
      const int64_t f = S.row_ptr[s + 1] - S.row_ptr[s];
      if (f > INT32_MAX) return "assembly records: a front's order is out of range";
      col_base[s] = ncols;
      ncols += f;
      A.unit_base[s] = nunits;
      nunits += f * ((f + chunk - 1) / chunk);
    }
  std::vector<int64_t> iptr(ncols + 1, 0);
  for (int c = 0; c < ns; ++c) {
    const int p = S.sn_parent[c];
    if (p < 0 || !big[p]) continue;
    for (int64_t q = S.rel_ptr[c]; q < S.rel_ptr[c + 1]; ++q) ++iptr[col_base[p] + S.rel[q] + 1];
  }
  for (int64_t i = 0; i < ncols; ++i) iptr[i + 1] += iptr[i];
  A.items = iptr[ncols];
  std::vector<int> ichild(A.items), ijj(A.items);
  {
    std::vector<int64_t> fill(iptr.begin(), iptr.end() - 1);
    for (int c = 0; c < ns; ++c) {
      const int p = S.sn_parent[c];
      if (p < 0 || !big[p]) continue;
      for (int64_t q = S.rel_ptr[c]; q < S.rel_ptr[c + 1]; ++q) {
        const int64_t slot = fill[col_base[p] + S.rel[q]]++;
        ichild[slot] = c;
        ijj[slot] = (int)(q - S.rel_ptr[c]);
      }
    }
  }
  // per child of a big front: where each chunk boundary of the parent falls in its (sorted) rel list
  std::vector<int64_t> cut_pos(ns, -1);
  std::vector<int> cutv;
  for (int c = 0; c < ns; ++c) {
    const int p = S.sn_parent[c];
    if (p < 0 || !big[p]) continue;
    const int64_t fp = S.row_ptr[p + 1] - S.row_ptr[p];
    const int* rb = S.rel.data() + S.rel_ptr[c];
    const int* re = S.rel.data() + S.rel_ptr[c + 1];
    cut_pos[c] = (int64_t)cutv.size();
    const int nchunks = (int)((fp + chunk - 1) / chunk);
    for (int t = 0; t <= nchunks; ++t) cutv.push_back((int)(std::lower_bound(rb, re, (int)std::min<int64_t>((int64_t)t * chunk, INT32_MAX)) - rb));
  }
  A.units.assign((size_t)nunits, AsmUnit{0, 0, 0, 0, {0, 0}});
  for (int s = 0; s < ns; ++s) {
    if (!big[s]) continue;
    const int64_t f = S.row_ptr[s + 1] - S.row_ptr[s];
    const int nchunks = (int)((f + chunk - 1) / chunk);
    const int64_t e0 = S.aent_ptr[s], e1 = S.aent_ptr[s + 1];
    const int64_t* dst = S.aent_dst.data();
    for (int t = 0; t < nchunks; ++t)
      for (int64_t pc = 0; pc < f; ++pc) {
        AsmUnit& U = A.units[(size_t)(A.unit_base[s] + (int64_t)t * f + pc)];
        U.piece0 = (int64_t)A.pieces.size();
        const int64_t r0 = std::max<int64_t>(pc, (int64_t)t * chunk), r1 = std::min<int64_t>(f, (int64_t)(t + 1) * chunk);
        if (r0 >= r1) continue;
        // A entries are sorted by destination lrow + lcol * f: the rows of column pc inside the chunk are one range
        const int64_t a0 = std::lower_bound(dst + e0, dst + e1, pc * f + r0) - dst;
        const int64_t a1 = std::lower_bound(dst + a0, dst + e1, pc * f + r1) - dst;
        U.a0 = a0;
        U.na = (int)(a1 - a0);
        for (int64_t q = iptr[col_base[s] + pc]; q < iptr[col_base[s] + pc + 1]; ++q) {
          const int c = ichild[q], jj = ijj[q];
          const int64_t fc = S.row_ptr[c + 1] - S.row_ptr[c];
          const int rc = (int)(fc - (S.sn_col0[c + 1] - S.sn_col0[c]));      // rows of the child's contribution block
          const int* cut = cutv.data() + cut_pos[c];
          const int lo = std::max(jj, cut[t]), hi = std::min(rc, cut[t + 1]);
          if (lo >= hi) continue;
          // column jj of the child's contribution block, its rows lo .. hi - 1
          A.pieces.push_back(AsmPiece{cb_base[c] + (int64_t)jj * fc + lo, (int)(S.rel_ptr[c] + lo), hi - lo});
        }
        U.np = (int)((int64_t)A.pieces.size() - U.piece0);
      }
  }
  return "";
}

}  // namespace okkt
