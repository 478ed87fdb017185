// C ABI, line-search batches (include/okkt.h: okkt_kkt_items_set_direction ... okkt_kkt_items_ls_query): the
// step-side functions of linesearch.hip for the items of a KKT batch, against the iterates and directions resident in the items' slots.
//
// Every kernel here is the body of its single-iterate twin (ls_device.h) on a grid with one more coordinate: blockIdx.y is the position
// in the item list, the slot items ? items[blockIdx.y] : blockIdx.y.  The partition is the twin's -- min(256, ceil(len / 1024))
// workgroups of 256 threads per item, grid-stride, partials at part[(slot * 256 + blockIdx.x) * NCH + c], one workgroup per item for the
// final pass -- and the scalars a map closes over in the twin are read from small device arrays indexed by slot, so item b is bit for
// bit what the single-iterate call returns for that iterate and direction on a handle of its own.  The products J dx, J'v and H dx are
// the batched row kernels of kkt_batch.hip, the host arithmetic behind the reductions is ls_finish.h.  No atomics, no workgroup waits
// for another.  Compiled with -ffp-contract=off, as linesearch.hip is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kkt_batch.h"
#include "kkt_state.h"
#include "ls_device.h"
#include "ls_finish.h"

using namespace okkt;

namespace {

__device__ __forceinline__ int64_t item_of(const int* __restrict__ items) { return items ? items[blockIdx.y] : (int)blockIdx.y; }
// scalar `row` of slot b; B: the reserved slots (the row length of KktLsSlots::scal)
#define LS_SC(row) (L.scal[(size_t)(row) * B + b])
#define LS_PART(nch) (L.part + (size_t)b * kLsMaxBlocks * (nch))

__global__ __launch_bounds__(256) void kb_ls_absmax(KktItemSlots S, KktLsSlots L, const int* __restrict__ items) {
  const int64_t b = item_of(items);
  ld_map_reduce<1>(S.n, MapAbs{S.dx + b * S.n}, Channels<1>{{kNanMax}, {0.0}}, LS_PART(1));
}
// frac: sm[0], stride fs (0: one vector for every item)
__global__ __launch_bounds__(256) void kb_ls_ratio_s(KktItemSlots S, KktLsSlots L, int64_t B, int64_t fs, const int* __restrict__ items) {
  const int64_t b = item_of(items), m = S.m;
  ld_map_reduce<1>(m, MapRatioS{S.s + b * m, S.ds + b * m, L.sm[0] + b * fs, S.s + b * m, LS_SC(kLsThr)}, Channels<1>{{kNanMax}, {1.0}}, LS_PART(1));
}
// s_new: sm[1]
__global__ __launch_bounds__(256) void kb_ls_s_bound(KktItemSlots S, KktLsSlots L, int64_t B, int64_t fs, const int* __restrict__ items) {
  const int64_t b = item_of(items), m = S.m;
  ld_map_reduce<1>(m, MapSBound{L.sm[1] + b * m, L.sm[0] + b * fs, S.s + b * m, LS_SC(kLsThr)}, Channels<1>{{kNanMin}, {1.0}}, LS_PART(1));
}
// s_cand: sm[1], y_cand: sm[2]; the item's `after` and the start of its ub channel from the scalars
__global__ __launch_bounds__(256) void kb_ls_dual_bounds(KktItemSlots S, KktLsSlots L, int64_t B, int64_t fs, double comp_feas, const int* __restrict__ items) {
  const int64_t b = item_of(items), m = S.m;
  const MapDualBounds f{L.sm[1] + b * m, L.sm[2] + b * m, S.dy + b * m, L.sm[0] + b * fs, S.y + b * m, LS_SC(kLsMu), comp_feas, LS_SC(kLsNxMin), (int64_t)LS_SC(kLsAfter)};
  ld_map_reduce<4>(m, f, Channels<4>{{kNanMax, kNanMin, kNanMax, kNanMax}, {0.0, LS_SC(kLsUbInit), -1.0, 1.0}}, LS_PART(4));
}
// v = J dx: sm[0]
__global__ __launch_bounds__(256) void kb_ls_pred_m(KktItemSlots S, KktLsSlots L, int64_t B, const int* __restrict__ items) {
  const int64_t b = item_of(items), m = S.m;
  const MapPredM f{L.sm[0] + b * m, S.s + b * m, S.y + b * m, S.dy + b * m, S.ds + b * m, LS_SC(kLsMu), LS_SC(kLsMuNew), LS_SC(kLsStep)};
  ld_map_reduce<3>(m, f, Channels<3>{{kSum, kNanMax, kNanMax}, {0.0, 0.0, 0.0}}, LS_PART(3));
}
// grad: sn[0], J'w: sn[1], H dx: the item's vn1
__global__ __launch_bounds__(256) void kb_ls_pred_n(KktItemSlots S, KktLsSlots L, const int* __restrict__ items) {
  const int64_t b = item_of(items), n = S.n;
  ld_map_reduce<2>(n, MapPredN{S.dx + b * n, L.sn[0] + b * n, L.sn[1] + b * n, S.vn1 + b * n}, Channels<2>{{kSum, kSum}, {0.0, 0.0}}, LS_PART(2));
}
// grad_cand: sn[0], J'(y - mu pen): sn[1], J'dy: the item's vn1
__global__ __launch_bounds__(256) void kb_ls_dual_n(KktItemSlots S, KktLsSlots L, int64_t B, const int* __restrict__ items) {
  const int64_t b = item_of(items), n = S.n;
  ld_map_reduce<2>(n, MapDualStepN{L.sn[0] + b * n, L.sn[1] + b * n, S.vn1 + b * n, LS_SC(kLsScaleD)}, Channels<2>{{kSum, kSum}, {0.0, 0.0}}, LS_PART(2));
}
__global__ __launch_bounds__(256) void kb_ls_dual_m(KktItemSlots S, KktLsSlots L, int64_t B, const int* __restrict__ items) {
  const int64_t b = item_of(items), m = S.m;
  ld_map_reduce<2>(m, MapDualStepM{L.sm[1] + b * m, L.sm[2] + b * m, S.dy + b * m, LS_SC(kLsScaleMu), LS_SC(kLsMu)}, Channels<2>{{kSum, kSum}, {0.0, 0.0}}, LS_PART(2));
}
// one workgroup per item: its nb partial rows into out[slot * 8 + off ...]; init1: the items' own start of channel 1 (the ub channel)
template <int NCH>
__global__ __launch_bounds__(256) void kb_ls_final(int nb, Channels<NCH> ch, const double* __restrict__ init1, KktLsSlots L, int off, const int* __restrict__ items) {
  const int64_t b = item_of(items);
  if constexpr (NCH > 1) { if (init1) ch.init[1] = init1[b]; }
  ld_reduce_final<NCH>(nb, ch, LS_PART(NCH), L.out + b * 8 + off);
}
// o_b = a_b * x_b + c_b (recip: a_b ./ x_b + c_b), a and c the items' kLsAxA / kLsAxB
__global__ void kb_ls_axpb(int64_t len, KktLsSlots L, int64_t B, const double* __restrict__ x, double* __restrict__ o, int recip, const int* __restrict__ items) {
  const int64_t b = item_of(items);
  ld_axpb(len, LS_SC(kLsAxA), x + b * len, LS_SC(kLsAxB), o + b * len, recip);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline int ls_blocks(int64_t len) { return (int)std::min<int64_t>(kLsMaxBlocks, (len + 1023) / 1024); }
inline dim3 grid1b(int64_t n, int64_t nl) { return dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256), (unsigned)nl); }

int64_t ls_slot_doubles(const okkt_kkt_s* k) { return 4 * k->m + 2 * k->n + kLsMaxBlocks * 8 + 8 + kLsScalars + k->nnzJ; }

template <typename T>
bool ls_alloc(KktItems* I, T** p, size_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
  I->allocs.push_back(q);
  *p = (T*)q;
  return true;
}

// one call of the family: the listed slots, the device list (NULL: slots 0 .. nl-1), the scalars of the slots
struct LsCall {
  okkt_kkt_s* k = nullptr;
  KktItems* I = nullptr;
  const char* what = "";
  int64_t B = 0, nl = 0;
  const int* d_list = nullptr;
  std::vector<int32_t> slots;
  std::vector<double> scal;      // [kLsScalars][I->B]
  double& sc(int row, int64_t b) { return scal[(size_t)row * (size_t)I->B + (size_t)b]; }
};

int ensure_ls_slots(okkt_kkt_s* k, const char* what) {
  KktItems* I = k->items;
  KktLsSlots& L = I->LS;
  if (L.ready) return OKKT_OK;
  const size_t b = (size_t)I->B, n = (size_t)k->n, m = (size_t)k->m;
  const bool ok = ls_alloc(I, &L.sm[0], b * m) && ls_alloc(I, &L.sm[1], b * m) && ls_alloc(I, &L.sm[2], b * m) && ls_alloc(I, &L.sm[3], b * m) &&
                  ls_alloc(I, &L.sn[0], b * n) && ls_alloc(I, &L.sn[1], b * n) && ls_alloc(I, &L.part, b * kLsMaxBlocks * 8) && ls_alloc(I, &L.out, b * 8) &&
                  ls_alloc(I, &L.scal, b * kLsScalars) && ls_alloc(I, &L.list, b);
  if (!ok)      // what was allocated stays in the reservation's list and goes with it
    return kk_fail(k, OKKT_ERR_ALLOC, std::string(what) + ": the line-search slots of " + std::to_string(I->B) + " items (" + std::to_string(ls_slot_doubles(k) * 8) +
                                          " bytes each) do not fit the device memory");
  L.ready = true;
  return OKKT_OK;
}

// the gate of the family, B against the formed items and those that hold a direction, the item list, the slots
int ls_begin(okkt_kkt_s* k, const char* what, int64_t B, const int32_t* items, int64_t nitems, LsCall* c) {
  if (!k) return OKKT_ERR_INVALID;
  int rc = kkt_items_gate(k, what, B);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  const std::string w(what);
  if (I->formed_B < 1) return kk_fail(k, OKKT_ERR_INVALID, w + ": okkt_kkt_items_form_system has not been called");
  if (B > I->formed_B) return kk_fail(k, OKKT_ERR_INVALID, w + ": B above the " + std::to_string(I->formed_B) + " items of the last okkt_kkt_items_form_system");
  if (B > I->dir_B)
    return kk_fail(k, OKKT_ERR_INVALID, "no direction: call okkt_kkt_items_compute_direction or okkt_kkt_items_set_direction for " + std::to_string(B) + " items first (" +
                                            std::to_string(I->dir_B) + " hold one)");
  c->k = k; c->I = I; c->what = what; c->B = B;
  if (items) {
    if (nitems < 0 || nitems > B) return kk_fail(k, OKKT_ERR_INVALID, w + ": nitems outside 0 .. B");
    std::vector<char> seen((size_t)B, 0);
    for (int64_t q = 0; q < nitems; ++q) {
      const int32_t b = items[q];
      if (b < 0 || b >= B) return kk_fail(k, OKKT_ERR_INVALID, w + ": item " + std::to_string(b) + " outside 0 .. B-1");
      if (seen[(size_t)b]) return kk_fail(k, OKKT_ERR_INVALID, w + ": item " + std::to_string(b) + " is listed twice");
      seen[(size_t)b] = 1;
    }
    c->slots.assign(items, items + nitems);
  } else {
    c->slots.resize((size_t)B);
    for (int64_t b = 0; b < B; ++b) c->slots[(size_t)b] = (int32_t)b;
  }
  c->nl = (int64_t)c->slots.size();
  if ((rc = ensure_ls_slots(k, what)) != OKKT_OK) return rc;
  c->d_list = items ? I->LS.list : nullptr;
  c->scal.assign((size_t)kLsScalars * (size_t)I->B, 0.0);
  return OKKT_OK;
}

int upload_list(LsCall& c, const std::vector<int32_t>& list) {
  okkt_kkt_s* k = c.k;
  if (!list.empty()) KK_TRY(k, hipMemcpyAsync(c.I->LS.list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, kk_stream(k)));
  return OKKT_OK;
}
int upload_scalars(LsCall& c) {
  okkt_kkt_s* k = c.k;
  KK_TRY(k, hipMemcpyAsync(c.I->LS.scal, c.scal.data(), c.scal.size() * 8, hipMemcpyHostToDevice, kk_stream(k)));
  return OKKT_OK;
}
// the rows of the listed slots of a host array [B][len] into dst; stride 0: the one row every item reads
int stage_rows(LsCall& c, double* dst, const double* src, int64_t len, bool shared, bool have_list) {
  okkt_kkt_s* k = c.k;
  hipStream_t st = kk_stream(k);
  if (len <= 0) return OKKT_OK;
  if (shared) { KK_TRY(k, hipMemcpyAsync(dst, src, (size_t)len * 8, hipMemcpyHostToDevice, st)); return OKKT_OK; }
  if (!have_list) { KK_TRY(k, hipMemcpyAsync(dst, src, (size_t)(c.B * len) * 8, hipMemcpyHostToDevice, st)); return OKKT_OK; }
  for (const int32_t b : c.slots) KK_TRY(k, hipMemcpyAsync(dst + (size_t)b * len, src + (size_t)b * len, (size_t)len * 8, hipMemcpyHostToDevice, st));
  return OKKT_OK;
}
// the results [B][8] to the host behind everything enqueued: the synchronisation of a pass
int fetch_out(LsCall& c, std::vector<double>* out) {
  okkt_kkt_s* k = c.k;
  hipStream_t st = kk_stream(k);
  out->assign((size_t)c.I->B * 8, 0.0);
  KK_TRY(k, hipMemcpyAsync(out->data(), c.I->LS.out, out->size() * 8, hipMemcpyDeviceToHost, st));
  KK_TRY(k, hipStreamSynchronize(st));
  KK_TRY(k, hipGetLastError());
  return OKKT_OK;
}

// norm(dx_b, Inf) of every item that holds a direction: one batched launch per direction, cached on the host
int ensure_dx_norms(LsCall& c) {
  okkt_kkt_s* k = c.k;
  KktItems* I = c.I;
  if (I->dxnorm_ok) return OKKT_OK;
  const int64_t nd = I->dir_B;
  I->dxnorm.assign((size_t)I->B, 0.0);
  if (k->n > 0) {
    hipStream_t st = kk_stream(k);
    const int nb = ls_blocks(k->n);
    hipLaunchKernelGGL(kb_ls_absmax, dim3((unsigned)nb, (unsigned)nd), dim3(256), 0, st, I->S, I->LS, (const int*)nullptr);
    hipLaunchKernelGGL((kb_ls_final<1>), dim3(1, (unsigned)nd), dim3(256), 0, st, nb, Channels<1>{{kNanMax}, {0.0}}, (const double*)nullptr, I->LS, 0, (const int*)nullptr);
    std::vector<double> out;
    const int rc = fetch_out(c, &out);
    if (rc != OKKT_OK) return rc;
    for (int64_t b = 0; b < nd; ++b) I->dxnorm[(size_t)b] = out[(size_t)b * 8];
  }
  I->dxnorm_ok = true;
  return OKKT_OK;
}

int bad_stride(okkt_kkt_s* k, const char* what) { return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": frac_stride must be 0 (one vector for every item) or m"); }
int null_array(okkt_kkt_s* k, const char* what) { return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": a required array is NULL"); }

}  // namespace

extern "C" {

int okkt_kkt_items_ls_query(okkt_kkt_handle k, okkt_kkt_items_ls_info* out) {
  if (!k || !out) return OKKT_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  okkt_kkt_items_info q;
  const int rc = okkt_kkt_items_query(k, &q);
  if (rc != OKKT_OK) return rc;
  out->eligible = q.eligible;
  out->reason = q.reason;
  if (!q.eligible) return OKKT_OK;
  const bool n = k->n > 0, m = k->m > 0;
  out->extra_bytes_per_item = ls_slot_doubles(k) * 8;
  out->launches_dx_norm = n ? 2 : 0;
  out->launches_max_step = m ? 2 : 0;
  out->launches_s_bound = m ? 2 : 0;
  out->launches_dual_range = m ? 2 : 0;                                         // per pass
  out->launches_predicted_reduction = (m ? 4 : 0) + (n ? (m ? 1 : 0) + 3 : 0);  // J dx, mu ./ s, map, final; J'w, H dx, map, final
  out->launches_dual_step = (n ? (m ? 3 : 0) + 2 : 0) + (m ? 2 : 0);            // y - mu pen, J'w, J'dy, map, final; map, final
  return OKKT_OK;
}

int okkt_kkt_items_set_direction(okkt_kkt_handle k, int64_t B, const double* dx, const double* dy, const double* ds) {
  if (!k) return OKKT_ERR_INVALID;
  const char* what = "okkt_kkt_items_set_direction";
  int rc = kkt_items_gate(k, what, B);
  if (rc != OKKT_OK) return rc;
  KktItems* I = k->items;
  if (I->formed_B < 1) return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": okkt_kkt_items_form_system has not been called");
  if (B > I->formed_B) return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": B above the " + std::to_string(I->formed_B) + " items of the last okkt_kkt_items_form_system");
  const int64_t n = k->n, m = k->m;
  if ((n > 0 && !dx) || (m > 0 && (!dy || !ds))) return null_array(k, what);
  hipStream_t st = kk_stream(k);
  if (n) KK_TRY(k, hipMemcpyAsync(I->S.dx, dx, (size_t)(B * n) * 8, hipMemcpyHostToDevice, st));
  if (m) {
    KK_TRY(k, hipMemcpyAsync(I->S.dy, dy, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
    KK_TRY(k, hipMemcpyAsync(I->S.ds, ds, (size_t)(B * m) * 8, hipMemcpyHostToDevice, st));
  }
  KK_TRY(k, hipStreamSynchronize(st));
  I->dir_B = B;
  I->solved_B = std::min(I->solved_B, B);
  I->dxnorm_ok = false;
  return OKKT_OK;
}

int okkt_kkt_items_max_step_primal(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* frac_bd_predict, int64_t frac_stride,
                                   double ex, double* step_size_P, double* dx_norm_inf) {
  const char* what = "okkt_kkt_items_max_step_primal";
  try {
    LsCall c;
    int rc = ls_begin(k, what, B, items, nitems, &c);
    if (rc != OKKT_OK) return rc;
    const int64_t m = k->m;
    if (!step_size_P || (m > 0 && !frac_bd_predict)) return null_array(k, what);
    if (frac_stride != 0 && frac_stride != m) return bad_stride(k, what);
    if (c.nl == 0) return OKKT_OK;
    if ((rc = ensure_dx_norms(c)) != OKKT_OK) return rc;
    KktItems* I = c.I;
    std::vector<double> out((size_t)I->B * 8, 1.0);
    if (m > 0) {
      for (const int32_t b : c.slots) c.sc(kLsThr, b) = thres_scalar(I->dxnorm[(size_t)b], ex);
      if ((rc = upload_list(c, items ? c.slots : std::vector<int32_t>())) != OKKT_OK || (rc = upload_scalars(c)) != OKKT_OK ||
          (rc = stage_rows(c, I->LS.sm[0], frac_bd_predict, m, frac_stride == 0, items != nullptr)) != OKKT_OK)
        return rc;
      hipStream_t st = kk_stream(k);
      const int nb = ls_blocks(m);
      hipLaunchKernelGGL(kb_ls_ratio_s, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, I->S, I->LS, I->B, frac_stride, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<1>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, Channels<1>{{kNanMax}, {1.0}}, (const double*)nullptr, I->LS, 0, c.d_list);
      if ((rc = fetch_out(c, &out)) != OKKT_OK) return rc;
    }
    for (const int32_t b : c.slots) {
      step_size_P[b] = step_from_ratio(out[(size_t)b * 8]);
      if (dx_norm_inf) dx_norm_inf[b] = I->dxnorm[(size_t)b];
    }
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, std::string("out of host memory in ") + what);
  }
}

int okkt_kkt_items_s_bound_ok(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* s_new, const double* frac_bd, int64_t frac_stride,
                              double ex, int32_t* ok) {
  const char* what = "okkt_kkt_items_s_bound_ok";
  try {
    LsCall c;
    int rc = ls_begin(k, what, B, items, nitems, &c);
    if (rc != OKKT_OK) return rc;
    const int64_t m = k->m;
    if (!ok || (m > 0 && (!s_new || !frac_bd))) return null_array(k, what);
    if (frac_stride != 0 && frac_stride != m) return bad_stride(k, what);
    if (c.nl == 0) return OKKT_OK;
    if ((rc = ensure_dx_norms(c)) != OKKT_OK) return rc;
    KktItems* I = c.I;
    std::vector<double> out((size_t)I->B * 8, 1.0);
    if (m > 0) {
      for (const int32_t b : c.slots) c.sc(kLsThr, b) = thres_scalar(I->dxnorm[(size_t)b], ex);
      if ((rc = upload_list(c, items ? c.slots : std::vector<int32_t>())) != OKKT_OK || (rc = upload_scalars(c)) != OKKT_OK ||
          (rc = stage_rows(c, I->LS.sm[0], frac_bd, m, frac_stride == 0, items != nullptr)) != OKKT_OK ||
          (rc = stage_rows(c, I->LS.sm[1], s_new, m, false, items != nullptr)) != OKKT_OK)
        return rc;
      hipStream_t st = kk_stream(k);
      const int nb = ls_blocks(m);
      hipLaunchKernelGGL(kb_ls_s_bound, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, I->S, I->LS, I->B, frac_stride, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<1>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, Channels<1>{{kNanMin}, {1.0}}, (const double*)nullptr, I->LS, 0, c.d_list);
      if ((rc = fetch_out(c, &out)) != OKKT_OK) return rc;
    }
    for (const int32_t b : c.slots) ok[b] = out[(size_t)b * 8] == 1.0 ? 1 : 0;
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, std::string("out of host memory in ") + what);
  }
}

int okkt_kkt_items_dual_step_range(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* s_cand, const double* y_cand,
                                   const double* mu_cand, double comp_feas, const double* frac_bd, int64_t frac_stride, double* lb_out, double* ub_out) {
  const char* what = "okkt_kkt_items_dual_step_range";
  try {
    LsCall c;
    int rc = ls_begin(k, what, B, items, nitems, &c);
    if (rc != OKKT_OK) return rc;
    const int64_t m = k->m;
    if (!lb_out || !ub_out || !mu_cand || (m > 0 && (!s_cand || !y_cand || !frac_bd))) return null_array(k, what);
    if (frac_stride != 0 && frac_stride != m) return bad_stride(k, what);
    if (c.nl == 0) return OKKT_OK;
    if ((rc = ensure_dx_norms(c)) != OKKT_OK) return rc;
    KktItems* I = c.I;
    // the identities of the four channels: what a launch over no entries leaves (m = 0)
    std::vector<double> out((size_t)I->B * 8, 0.0);
    for (const int32_t b : c.slots) { double* r = out.data() + (size_t)b * 8; r[0] = 0.0; r[1] = 1.0; r[2] = -1.0; r[3] = 1.0; }
    if (m > 0) {
      // pass 1 over the listed items: lb = max over the entries (start 0), ub = min (start 1), the last reset index, and the ratio of
      // simple_max_step(y_cand, dy, lb_y)
      for (const int32_t b : c.slots) {
        c.sc(kLsMu, b) = mu_cand[b];
        c.sc(kLsNxMin, b) = jl_min(1.0, I->dxnorm[(size_t)b]);
        c.sc(kLsAfter, b) = -1.0;
        c.sc(kLsUbInit, b) = 1.0;
      }
      if ((rc = upload_list(c, items ? c.slots : std::vector<int32_t>())) != OKKT_OK || (rc = upload_scalars(c)) != OKKT_OK ||
          (rc = stage_rows(c, I->LS.sm[0], frac_bd, m, frac_stride == 0, items != nullptr)) != OKKT_OK ||
          (rc = stage_rows(c, I->LS.sm[1], s_cand, m, false, items != nullptr)) != OKKT_OK ||
          (rc = stage_rows(c, I->LS.sm[2], y_cand, m, false, items != nullptr)) != OKKT_OK)
        return rc;
      hipStream_t st = kk_stream(k);
      const int nb = ls_blocks(m);
      const Channels<4> ch{{kNanMax, kNanMin, kNanMax, kNanMax}, {0.0, 1.0, -1.0, 1.0}};
      const double* ubinit = I->LS.scal + (size_t)kLsUbInit * (size_t)I->B;
      hipLaunchKernelGGL(kb_ls_dual_bounds, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, I->S, I->LS, I->B, frac_stride, comp_feas, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<4>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, ch, ubinit, I->LS, 0, c.d_list);
      if ((rc = fetch_out(c, &out)) != OKKT_OK) return rc;
      // pass 2 over the items in which an entry with dy == 0 reset the interval to (0, -1): only what follows the item's last reset
      // counts, its ub channel starts at -1, and the ratio of pass 1 is kept
      std::vector<int32_t> again;
      for (const int32_t b : c.slots) {
        const double* r = out.data() + (size_t)b * 8;
        if (r[2] >= 0.0) {
          again.push_back(b);
          c.sc(kLsAfter, b) = (double)(int64_t)r[2];
          c.sc(kLsUbInit, b) = -1.0;
        }
      }
      if (!again.empty()) {
        if ((rc = upload_list(c, again)) != OKKT_OK || (rc = upload_scalars(c)) != OKKT_OK) return rc;
        const unsigned na = (unsigned)again.size();
        hipLaunchKernelGGL(kb_ls_dual_bounds, dim3((unsigned)nb, na), dim3(256), 0, st, I->S, I->LS, I->B, frac_stride, comp_feas, (const int*)I->LS.list);
        hipLaunchKernelGGL((kb_ls_final<4>), dim3(1, na), dim3(256), 0, st, nb, ch, ubinit, I->LS, 0, (const int*)I->LS.list);
        std::vector<double> out2;
        if ((rc = fetch_out(c, &out2)) != OKKT_OK) return rc;
        for (const int32_t b : again) {
          double* r = out.data() + (size_t)b * 8;
          const double ratio_y = r[3];
          std::memcpy(r, out2.data() + (size_t)b * 8, 4 * sizeof(double));
          r[3] = ratio_y;
        }
      }
    }
    for (const int32_t b : c.slots) dual_range_finish(out.data() + (size_t)b * 8, lb_out + b, ub_out + b);
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, std::string("out of host memory in ") + what);
  }
}

int okkt_kkt_items_predicted_reduction(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* grad, const double* mu, const double* dmu,
                                       const double* a_norm_penalty, const double* step_size, double* out4) {
  const char* what = "okkt_kkt_items_predicted_reduction";
  try {
    LsCall c;
    int rc = ls_begin(k, what, B, items, nitems, &c);
    if (rc != OKKT_OK) return rc;
    const int64_t n = k->n, m = k->m;
    if (!out4 || !mu || !dmu || !a_norm_penalty || !step_size || (n > 0 && !grad)) return null_array(k, what);
    if (c.nl == 0) return OKKT_OK;
    KktItems* I = c.I;
    KktItemSlots& S = I->S;
    KktLsSlots& L = I->LS;
    hipStream_t st = kk_stream(k);
    for (const int32_t b : c.slots) {
      c.sc(kLsMu, b) = mu[b];
      c.sc(kLsMuNew, b) = mu[b] + dmu[b] * step_size[b];
      c.sc(kLsStep, b) = step_size[b];
      c.sc(kLsAxA, b) = mu[b];                              // eval_grad_phi = grad - J'(mu ./ s - mu * pen)
      c.sc(kLsAxB, b) = -(mu[b] * a_norm_penalty[b]);
    }
    if ((rc = upload_list(c, items ? c.slots : std::vector<int32_t>())) != OKKT_OK || (rc = upload_scalars(c)) != OKKT_OK ||
        (rc = stage_rows(c, L.sn[0], grad, n, false, items != nullptr)) != OKKT_OK)
      return rc;
    // the m-part into out[slot][0 .. 2], the n-part into out[slot][4 .. 5]: one synchronisation for both
    if (m) {
      kkt_items_spmv(k, k->lprJr, m, c.nl, k->Jrp, k->Jrj, S.Jcsr, S.nnzJ, S.dx, n, L.sm[0], m, c.d_list);                      // v = J dx
      hipLaunchKernelGGL(kb_ls_axpb, grid1b(m, c.nl), dim3(256), 0, st, m, L, I->B, (const double*)S.s, L.sm[1], 1, c.d_list);
      const int nb = ls_blocks(m);
      hipLaunchKernelGGL(kb_ls_pred_m, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, S, L, I->B, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<3>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, Channels<3>{{kSum, kNanMax, kNanMax}, {0.0, 0.0, 0.0}}, (const double*)nullptr, L, 0,
                         c.d_list);
    }
    if (n) {
      if (m) kkt_items_spmv(k, k->lprJc, n, c.nl, k->Jp, k->Ji, S.Jx, S.Jx_stride, L.sm[1], m, L.sn[1], n, c.d_list);
      else KK_TRY(k, hipMemsetAsync(L.sn[1], 0, (size_t)(I->B * n) * 8, st));
      kkt_items_hess(k, c.nl, S.dx, n, S.vn1, n, c.d_list);
      const int nb = ls_blocks(n);
      hipLaunchKernelGGL(kb_ls_pred_n, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, S, L, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<2>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, Channels<2>{{kSum, kSum}, {0.0, 0.0}}, (const double*)nullptr, L, 4, c.d_list);
    }
    std::vector<double> out;
    if (m || n) {
      if ((rc = fetch_out(c, &out)) != OKKT_OK) return rc;
    } else {
      out.assign((size_t)I->B * 8, 0.0);
    }
    for (const int32_t b : c.slots) {
      const double* r = out.data() + (size_t)b * 8;
      const double rm[3] = {m ? r[0] : 0.0, m ? r[1] : 0.0, m ? r[2] : 0.0}, rn[2] = {n ? r[4] : 0.0, n ? r[5] : 0.0};
      predicted_reduction_finish(m, rm, rn, mu[b], step_size[b], out4 + (size_t)b * 4);
    }
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, std::string("out of host memory in ") + what);
  }
}

int okkt_kkt_items_dual_step(okkt_kkt_handle k, int64_t B, const int32_t* items, int64_t nitems, const double* J_nzval_cand, int64_t J_stride, const double* grad_cand,
                             const double* s_cand, const double* y_cand, const double* mu_cand, const double* a_norm_penalty, const double* step_size_P,
                             const double* lb, const double* ub, const double* scale_D, const double* scale_mu, int dual_ls, double* step_size_D) {
  const char* what = "okkt_kkt_items_dual_step";
  try {
    LsCall c;
    int rc = ls_begin(k, what, B, items, nitems, &c);
    if (rc != OKKT_OK) return rc;
    if (!step_size_D || !ub) return null_array(k, what);
    if (dual_ls != 1 && dual_ls != 3) {
      for (const int32_t b : c.slots) step_size_D[b] = ub[b];
      return OKKT_OK;
    }
    const int64_t n = k->n, m = k->m;
    if (!mu_cand || !a_norm_penalty || !step_size_P || !lb || !scale_D || !scale_mu || (n > 0 && !grad_cand) || (m > 0 && (!s_cand || !y_cand)))
      return null_array(k, what);
    const bool own_J = J_nzval_cand && k->nnzJ;
    if (own_J && J_stride != 0 && J_stride < k->nnzJ)
      return kk_fail(k, OKKT_ERR_INVALID, std::string(what) + ": J_stride must be 0 (one array for every item) or at least the number of entries");
    if (c.nl == 0) return OKKT_OK;
    KktItems* I = c.I;
    KktItemSlots& S = I->S;
    KktLsSlots& L = I->LS;
    hipStream_t st = kk_stream(k);
    const double* Jx = S.Jx;
    int64_t Jxs = S.Jx_stride;
    if (own_J) {
      const int64_t need = J_stride ? I->B : 1;
      if (L.Jcand_cap < need) {
        L.Jcand_cap = 0;
        if (!ls_alloc(I, &L.Jcand, (size_t)need * (size_t)k->nnzJ))
          return kk_fail(k, OKKT_ERR_ALLOC, std::string(what) + ": " + std::to_string(need) + " arrays of " + std::to_string(k->nnzJ * 8) + " bytes do not fit the device memory");
        L.Jcand_cap = need;
      }
      const size_t row = (size_t)k->nnzJ * 8;
      if (J_stride == 0) KK_TRY(k, hipMemcpyAsync(L.Jcand, J_nzval_cand, row, hipMemcpyHostToDevice, st));
      else if (!items && J_stride == k->nnzJ) KK_TRY(k, hipMemcpyAsync(L.Jcand, J_nzval_cand, row * (size_t)B, hipMemcpyHostToDevice, st));
      else
        for (const int32_t b : c.slots) KK_TRY(k, hipMemcpyAsync(L.Jcand + (size_t)b * k->nnzJ, J_nzval_cand + (size_t)b * J_stride, row, hipMemcpyHostToDevice, st));
      Jx = L.Jcand;
      Jxs = J_stride ? k->nnzJ : 0;
    }
    for (const int32_t b : c.slots) {
      c.sc(kLsMu, b) = mu_cand[b];
      c.sc(kLsScaleD, b) = scale_D[b];
      c.sc(kLsScaleMu, b) = scale_mu[b];
      c.sc(kLsAxA, b) = 1.0;                                // eval_grad_lag(new_it, mu) = grad - J'(y - mu * pen)
      c.sc(kLsAxB, b) = -(mu_cand[b] * a_norm_penalty[b]);
    }
    if ((rc = upload_list(c, items ? c.slots : std::vector<int32_t>())) != OKKT_OK || (rc = upload_scalars(c)) != OKKT_OK ||
        (rc = stage_rows(c, L.sn[0], grad_cand, n, false, items != nullptr)) != OKKT_OK ||
        (rc = stage_rows(c, L.sm[1], s_cand, m, false, items != nullptr)) != OKKT_OK ||
        (rc = stage_rows(c, L.sm[2], y_cand, m, false, items != nullptr)) != OKKT_OK)
      return rc;
    // the n-part into out[slot][0 .. 1], the m-part into out[slot][4 .. 5]
    if (n) {
      if (m) {
        hipLaunchKernelGGL(kb_ls_axpb, grid1b(m, c.nl), dim3(256), 0, st, m, L, I->B, (const double*)L.sm[2], L.sm[3], 0, c.d_list);
        kkt_items_spmv(k, k->lprJc, n, c.nl, k->Jp, k->Ji, Jx, Jxs, L.sm[3], m, L.sn[1], n, c.d_list);
        kkt_items_spmv(k, k->lprJc, n, c.nl, k->Jp, k->Ji, Jx, Jxs, S.dy, m, S.vn1, n, c.d_list);
      } else {
        KK_TRY(k, hipMemsetAsync(L.sn[1], 0, (size_t)(I->B * n) * 8, st));
        KK_TRY(k, hipMemsetAsync(S.vn1, 0, (size_t)(I->B * n) * 8, st));
      }
      const int nb = ls_blocks(n);
      hipLaunchKernelGGL(kb_ls_dual_n, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, S, L, I->B, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<2>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, Channels<2>{{kSum, kSum}, {0.0, 0.0}}, (const double*)nullptr, L, 0, c.d_list);
    }
    if (m) {
      const int nb = ls_blocks(m);
      hipLaunchKernelGGL(kb_ls_dual_m, dim3((unsigned)nb, (unsigned)c.nl), dim3(256), 0, st, S, L, I->B, c.d_list);
      hipLaunchKernelGGL((kb_ls_final<2>), dim3(1, (unsigned)c.nl), dim3(256), 0, st, nb, Channels<2>{{kSum, kSum}, {0.0, 0.0}}, (const double*)nullptr, L, 4, c.d_list);
    }
    std::vector<double> out;
    if (m || n) {
      if ((rc = fetch_out(c, &out)) != OKKT_OK) return rc;
    } else {
      out.assign((size_t)I->B * 8, 0.0);
    }
    for (const int32_t b : c.slots) {
      const double* r = out.data() + (size_t)b * 8;
      const double rn[2] = {n ? r[0] : 0.0, n ? r[1] : 0.0}, rm[2] = {m ? r[4] : 0.0, m ? r[5] : 0.0};
      step_size_D[b] = dual_step_finish(rn, rm, ub[b], dual_small_step(lb[b], ub[b], step_size_P[b]));
    }
    return OKKT_OK;
  } catch (const std::bad_alloc&) {
    return kk_fail(k, OKKT_ERR_ALLOC, std::string("out of host memory in ") + what);
  }
}

}  // extern "C"
