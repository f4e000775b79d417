// Instance tracking ("instance tracking" in centerpoly_hip.h) for gfx950: link the instances of one frame to the tracks
// of the frames before it by the IoU of their owned pixels, on the device, nothing read back between the stages.
//   cp_map_pairs        the hot path, two launches: a clear, then one streaming pass over a 16-bit map and a byte map
//                       that counts every (row, column) pair.  One workgroup per CU over a span of pixels, 16 pixels per
//                       lane and step, ONE run (row, column, count) per lane in registers; a counter is touched only
//                       when the pair changes.  Two regimes, the same for every lane of a launch:
//                         dense   (R + 1) * (n + 1) <= kLdsCells (33153 cells, 129.5 KB of the CU's 160 KB: the
//                                 tracker's whole range, 256 slots x 128 instances): the workgroup's table lives in LDS
//                                 and its non-zero cells go to the global table at the end, one atomic per cell.  The
//                                 grid is one workgroup per CU, so the LDS one workgroup claims costs no residency.
//                         sparse  otherwise (up to 1025 x 256 cells, 1 MB): every run goes straight to the global
//                                 table, which stays in L2.
//   cp_track_associate  ONE workgroup, one lane per slot: areas from the pair table, then the greedy matching -- every
//                       lane keeps the best candidate of its row, one wave picks the best of all, the lanes whose
//                       candidate lost its column look again -- then new tracks, ageing and the commit.
//   cp_track_update     one pass: the memory map and the id image from two small tables in LDS.
// Integer atomics only in the counting: the counts do not depend on the order of the additions.  The IoU order is
// decided on 64-bit integer products; the threshold is one float64 division.
// The piece, span and run scheme, the loaders and the run walker are pixel_pieces.h's.
#include "pixel_pieces.h"

namespace {

constexpr int kMaxRows = 1024, kMaxCols = 255;
constexpr int kSlots = 256, kMaxInst = 128;             // CP_TRACK_SLOTS, instances per frame
constexpr int kWorkgroups = 256;                        // one per CU
constexpr int kLdsCells = (kSlots + 1) * (kMaxInst + 1);  // dense regime: 33153 counters per workgroup
constexpr unsigned kNone = 0xffff;
constexpr int kSlotInts = 5, kInstInts = 5;             // {track_id, label, first_frame, last_seen, hits}, {slot, ...}

struct PairArgs {
  const uint16_t* a;          // [HW]
  const uint16_t* row_of;     // [65536] or null
  const uint8_t* b;           // [HW]
  int* pairs;                 // [R + 1][n + 1]
  long long HW, span;         // pixels, pixels per workgroup (a multiple of kTile)
  int R, n;
};

struct InstTable {
  int label[kMaxInst];
  uint8_t live[kMaxInst];
};

__global__ __launch_bounds__(kThreads) void pairs_clear_kernel(int* __restrict__ pairs, int cells) {
  for (int k = blockIdx.x * kThreads + threadIdx.x; k < cells; k += gridDim.x * kThreads) pairs[k] = 0;
}

__global__ __launch_bounds__(kThreads) void map_pairs_kernel(PairArgs q) {
  __shared__ unsigned cells[kLdsCells];
  const int C = q.n + 1, used = (q.R + 1) * C;
  const bool dense = used <= kLdsCells;                                   // the same for every lane of the launch
  if (dense) {
    for (int k = threadIdx.x; k < used; k += kThreads) cells[k] = 0;
    __syncthreads();
  }
  const bool fast_a = aligned16(q.a), fast_b = aligned16(q.b);
  PairRun run;                                                            // the lane's run: value of a, column
  unsigned run_row = 0;                                                   // the value's row
  auto look = [&](bool a_changed, bool) {
    if (a_changed) run_row = min(q.row_of ? (unsigned)q.row_of[run.a] : (unsigned)run.a, (unsigned)q.R);
  };
  auto flush = [&](unsigned cnt) {
    const int cell = (int)run_row * C + run.b;
    if (dense) atomicAdd(&cells[cell], cnt);
    else atomicAdd(&q.pairs[cell], (int)cnt);
  };
  for_pieces(q.HW, q.span, [&](long long p0, int valid) {
    int v[kPiece], c[kPiece];
    load_ids(q.a, p0, valid, fast_a, v);
    load_bytes<false>(q.b + p0, valid, fast_b, c);
#pragma unroll
    for (int k = 0; k < kPiece; ++k) c[k] = min(c[k], q.n);
    walk_pairs(run, v, c, valid, look, flush);
  });
  if (run.cnt) flush(run.cnt);
  if (dense) {
    __syncthreads();
    for (int k = threadIdx.x; k < used; k += kThreads) {
      const unsigned cnt = cells[k];
      if (cnt) atomicAdd(&q.pairs[k], (int)cnt);
    }
  }
}

// a / b > c / d for positive denominators, exactly
__device__ __forceinline__ bool frac_gt(int a, int b, int c, int d) { return (long long)a * d > (long long)c * b; }

__global__ __launch_bounds__(kSlots) void track_associate_kernel(InstTable h, const int* __restrict__ pairs, int n,
                                                                 int* __restrict__ slots, int* __restrict__ next_id,
                                                                 double iou_thresh, int max_age, int t,
                                                                 int* __restrict__ inst, uint8_t* __restrict__ assigned,
                                                                 int* __restrict__ status) {
  __shared__ int s_slot[kSlots][kSlotInts];
  __shared__ int s_area_mem[kSlots], s_area_cur[kMaxInst];
  __shared__ int s_inst[kMaxInst][kInstInts];
  __shared__ int s_cand_inter[kSlots], s_cand_union[kSlots], s_cand_k[kSlots];   // a row's best candidate; inter 0: none
  __shared__ uint8_t s_assigned[kSlots];
  __shared__ int s_win, s_next, s_status;
  const int s = threadIdx.x, C = n + 1;
#pragma unroll
  for (int j = 0; j < kSlotInts; ++j) s_slot[s][j] = slots[kSlotInts * s + j];
  s_area_mem[s] = 0;
  s_assigned[s] = 0;
  if (s < kMaxInst) {
    s_area_cur[s] = 0;
    s_inst[s][0] = -1; s_inst[s][1] = 0; s_inst[s][2] = 0; s_inst[s][3] = 0; s_inst[s][4] = 0;
  }
  if (s == 0) { s_next = next_id[0]; s_status = 0; }
  __syncthreads();
  // the areas: ONE coalesced pass over the table, the none row and column included
  const int cells = (kSlots + 1) * C;
  for (int base = 0; base < cells; base += 8 * kSlots) {                  // (eight loads in flight per lane)
    int cnt[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = base + u * kSlots + s;
      cnt[u] = f < cells ? pairs[f] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (cnt[u] == 0) continue;
      const int f = base + u * kSlots + s, r = f / C, c = f - r * C;
      if (r < kSlots) atomicAdd(&s_area_mem[r], cnt[u]);
      if (c < n) atomicAdd(&s_area_cur[c], cnt[u]);
    }
  }
  __syncthreads();
  const int tid = s_slot[s][0], label = s_slot[s][1], area = s_area_mem[s];
  bool open = tid != 0;                                                   // this row can still match
  bool look = true;
  for (;;) {
    if (open && look) {                                                   // the row's best free candidate, ascending k
      int bi = 0, bu = 1, bk = -1;
      for (int k0 = 0; k0 < n; k0 += 8) {                                  // eight cells of the row in flight
        int cnt[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cnt[u] = k0 + u < n ? pairs[s * C + k0 + u] : 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + u, inter = cnt[u];
          if (inter <= 0 || !h.live[k] || h.label[k] != label || s_inst[k][0] >= 0) continue;
          const int uni = area + s_area_cur[k] - inter;
          if (!((double)inter / (double)uni >= iou_thresh)) continue;
          if (bk < 0 || frac_gt(inter, uni, bi, bu)) { bi = inter; bu = uni; bk = k; }
        }
      }
      if (bk < 0) open = false;
      s_cand_inter[s] = bk < 0 ? 0 : bi; s_cand_union[s] = bu; s_cand_k[s] = bk;
      look = false;
    } else if (!open) {
      s_cand_inter[s] = 0;
    }
    __syncthreads();
    if (s < CP_WAVE) {                                                    // the first wave: the best of all rows
      int wi = 0, wu = 1, wt = 0, ws = -1;
      for (int r = s; r < kSlots; r += CP_WAVE) {
        const int ci = s_cand_inter[r];
        if (ci == 0) continue;
        const int cu = s_cand_union[r], ct = s_slot[r][0];
        if (ws < 0 || frac_gt(ci, cu, wi, wu) || (!frac_gt(wi, wu, ci, cu) && ct < wt)) { wi = ci; wu = cu; wt = ct; ws = r; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int oi = __shfl_xor(wi, o, CP_WAVE), ou = __shfl_xor(wu, o, CP_WAVE);
        const int ot = __shfl_xor(wt, o, CP_WAVE), os = __shfl_xor(ws, o, CP_WAVE);
        if (os >= 0 && (ws < 0 || frac_gt(oi, ou, wi, wu) || (!frac_gt(wi, wu, oi, ou) && ot < wt))) {
          wi = oi; wu = ou; wt = ot; ws = os;
        }
      }
      if (s == 0) {
        s_win = ws;
        if (ws >= 0) {
          const int k = s_cand_k[ws];
          s_inst[k][0] = ws; s_inst[k][1] = wt; s_inst[k][2] = wi; s_inst[k][3] = wu;
          s_assigned[ws] = 1;
        }
      }
    }
    __syncthreads();
    const int win = s_win;
    if (win < 0) break;
    const int won_k = s_cand_k[win];
    if (s == win) open = false;
    else if (open && s_cand_k[s] == won_k) look = true;
    __syncthreads();                                                      // s_win and the candidates are read: next round
  }
  if (s == 0) {                                                           // new tracks, ascending k, lowest free slot
    int f = 0;
    for (int k = 0; k < n; ++k) {
      if (!h.live[k] || s_inst[k][0] >= 0) continue;
      while (f < kSlots && s_slot[f][0] != 0) ++f;
      if (f == kSlots) { s_status = 1; break; }
      const int id = s_next++;
      s_slot[f][0] = id; s_slot[f][1] = h.label[k]; s_slot[f][2] = t; s_slot[f][3] = t - 1; s_slot[f][4] = 0;
      s_inst[k][0] = f; s_inst[k][1] = id; s_inst[k][4] = 1;
      s_assigned[f] = 1;
    }
  }
  __syncthreads();
  if (s_status) {                                                         // mem and the table stay as they were
    if (s == 0) status[0] = 1;
    return;
  }
  if (s_assigned[s]) { s_slot[s][3] = t; s_slot[s][4] += 1; }
  const bool freed = s_slot[s][0] != 0 && (long long)s_slot[s][3] < (long long)t - max_age;
#pragma unroll
  for (int j = 0; j < kSlotInts; ++j) slots[kSlotInts * s + j] = freed ? 0 : s_slot[s][j];
  assigned[s] = s_assigned[s];
  if (s < n) {
#pragma unroll
    for (int j = 0; j < kInstInts; ++j) inst[kInstInts * s + j] = s_inst[s][j];
  }
  if (s == 0) { next_id[0] = s_next; status[0] = 0; }
}

struct UpdateArgs {
  const uint8_t* index;       // [HW]
  const int* slots;           // [256][5]
  const int* inst;            // [n][5]
  const uint8_t* assigned;    // [256]
  const int* status;
  uint16_t* mem;              // [HW]
  int* ids;                   // [HW]
  long long HW, span;
  int n, multiplier;
};

__global__ __launch_bounds__(kThreads) void track_update_kernel(InstTable h, UpdateArgs q) {
  __shared__ int s_col_id[256];                                           // label * multiplier + track id of a column
  __shared__ unsigned short s_col_slot[256];                              // its slot, kNone for no owner
  __shared__ uint8_t s_keep[kSlots];                                      // occupied and not assigned in this frame
  if (q.status[0]) return;
  const int t = threadIdx.x;
  const bool owner = t < q.n && q.inst[kInstInts * t] >= 0;
  s_col_slot[t] = owner ? (unsigned short)q.inst[kInstInts * t] : (unsigned short)kNone;
  s_col_id[t] = owner ? h.label[t] * q.multiplier + q.inst[kInstInts * t + 1] : 0;
  s_keep[t] = q.slots[kSlotInts * t] != 0 && !q.assigned[t];
  __syncthreads();
  const bool fast_index = aligned16(q.index), fast_mem = aligned16(q.mem), fast_ids = aligned16(q.ids);
  for_pieces(q.HW, q.span, [&](long long p0, int valid) {
    int v[kPiece], c[kPiece], id[kPiece];
    load_ids(q.mem, p0, valid, fast_mem, v);
    load_bytes<false>(q.index + p0, valid, fast_index, c);
#pragma unroll
    for (int k = 0; k < kPiece; ++k) {
      const unsigned slot = s_col_slot[c[k]];
      id[k] = s_col_id[c[k]];
      v[k] = slot != kNone ? (int)slot : (v[k] < kSlots && s_keep[v[k]] ? v[k] : (int)kNone);
    }
    if (valid == kPiece && fast_mem) {
      unsigned w[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = (unsigned)v[2 * k] | (unsigned)v[2 * k + 1] << 16;
      *reinterpret_cast<uint4*>(q.mem + p0) = make_uint4(w[0], w[1], w[2], w[3]);
      *reinterpret_cast<uint4*>(q.mem + p0 + 8) = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
#pragma unroll
      for (int k = 0; k < kPiece; ++k)
        if (k < valid) q.mem[p0 + k] = (uint16_t)v[k];
    }
    if (valid == kPiece && fast_ids) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        *reinterpret_cast<int4*>(q.ids + p0 + 4 * k) = make_int4(id[4 * k], id[4 * k + 1], id[4 * k + 2], id[4 * k + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < kPiece; ++k)
        if (k < valid) q.ids[p0 + k] = id[k];
    }
  });
}

void fill_inst_table(InstTable& h, int n, const int32_t* label, const uint8_t* live) {
  for (int k = 0; k < kMaxInst; ++k) {
    h.label[k] = k < n ? label[k] : 0;
    h.live[k] = k < n && (!live || live[k]) ? 1 : 0;
  }
}

}  // namespace

extern "C" int cp_map_pairs(const uint16_t* a, const uint16_t* row_of, int32_t R, const uint8_t* b, int32_t n, int32_t H,
                            int32_t W, int32_t* pairs, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && R >= 0 && n >= 0);
  const long long HW = (long long)H * W;
  if (R > kMaxRows || n > kMaxCols || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(a && b && pairs);
  CP_CHECK_ARG(((uintptr_t)a & 1) == 0 && ((uintptr_t)row_of & 1) == 0 && ((uintptr_t)pairs & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int cells = (R + 1) * (n + 1);
  hipLaunchKernelGGL(pairs_clear_kernel, dim3(min((cells + kThreads - 1) / kThreads, kWorkgroups)), dim3(kThreads), 0, st,
                     pairs, cells);
  PairArgs q;
  q.a = a; q.row_of = row_of; q.b = b; q.pairs = pairs; q.HW = HW; q.span = span_for(HW, kWorkgroups); q.R = R; q.n = n;
  hipLaunchKernelGGL(map_pairs_kernel, dim3(span_blocks(HW, q.span)), dim3(kThreads), 0, st, q);
  return cp_launch_status();
}

extern "C" int cp_track_associate(const int32_t* pairs, int32_t n, const int32_t* label, const uint8_t* live,
                                  int32_t* slots, int32_t* next_id, double iou_thresh, int32_t max_age, int32_t t,
                                  int32_t* inst, uint8_t* assigned, int32_t* status, void* stream) {
  CP_CHECK_ARG(n >= 0 && max_age >= 0 && t >= 0 && iou_thresh > 0 && iou_thresh <= 1);   // (a NaN fails both)
  if (n > kMaxInst) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(pairs && slots && next_id && assigned && status && (n == 0 || (label && live && inst)));
  CP_CHECK_ARG(((uintptr_t)pairs & 3) == 0 && ((uintptr_t)slots & 3) == 0 && ((uintptr_t)next_id & 3) == 0 &&
               ((uintptr_t)inst & 3) == 0 && ((uintptr_t)status & 3) == 0);
  InstTable h;
  fill_inst_table(h, n, label, live);
  hipLaunchKernelGGL(track_associate_kernel, dim3(1), dim3(kSlots), 0, (hipStream_t)stream, h, pairs, n, slots, next_id,
                     iou_thresh, max_age, t, inst, assigned, status);
  return cp_launch_status();
}

extern "C" int cp_track_update(const uint8_t* index, int32_t n, const int32_t* label, int32_t H, int32_t W,
                               const int32_t* slots, const int32_t* inst, const uint8_t* assigned, const int32_t* status,
                               int32_t multiplier, uint16_t* mem, int32_t* ids, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && n >= 0 && multiplier >= 1);
  const long long HW = (long long)H * W;
  if (n > kMaxInst || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(index && slots && assigned && status && mem && ids && (n == 0 || (label && inst)));
  CP_CHECK_ARG(((uintptr_t)slots & 3) == 0 && ((uintptr_t)inst & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
               ((uintptr_t)mem & 1) == 0 && ((uintptr_t)ids & 3) == 0);
  InstTable h;
  fill_inst_table(h, n, label, nullptr);
  UpdateArgs q;
  q.index = index; q.slots = slots; q.inst = inst; q.assigned = assigned; q.status = status; q.mem = mem; q.ids = ids;
  q.HW = HW; q.span = span_for(HW, 4 * kWorkgroups); q.n = n; q.multiplier = multiplier;
  hipLaunchKernelGGL(track_update_kernel, dim3(span_blocks(HW, q.span)), dim3(kThreads), 0, (hipStream_t)stream, h, q);
  return cp_launch_status();
}
