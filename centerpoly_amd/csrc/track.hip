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
// With motion ("instance tracking with motion"): cp_track_predict (a shift per slot), cp_map_pairs_shifted (the pair
// pass with every row's pixels read at the shifted position) and cp_track_kinematics (centroids and velocities) beside
// the three above, which stay as they are.
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

// ---- tracks predicted at constant velocity ("instance tracking with motion" in centerpoly_hip.h) ----
constexpr int kKinInts = 6;                             // {cx, cy, vx, vy, seen, valid}, positions in 1/16 pixel
constexpr int kMaxSide = 1 << 26;                       // 16 * x stays inside int32

struct ShiftArgs {
  const uint16_t* a;          // [HW]
  const int* shift;           // [R][2] = {dx, dy}
  const uint8_t* b;           // [HW]
  int* pairs;                 // [R + 1][n + 1]
  long long HW, span;
  int R, n, H, W;
};

// cp_map_pairs with every row's pixels moved by the row's shift before the byte map is read.  One pass, two runs per
// lane: the gathered pair (row, column at the shifted position) and the plain column of the lane's own pixels, which
// gives area_cur in row R; row R then loses the column sums of the rows above it.  A piece of 16 pixels of one row of
// the image and one row of the table reads its 16 bytes of `b` in one load at whatever byte offset the shift gives;
// every other piece that holds a track reads a byte per pixel.
__global__ __launch_bounds__(kThreads) void map_pairs_shifted_kernel(ShiftArgs q) {
  __shared__ unsigned cells[kLdsCells];
  __shared__ int2 s_shift[kMaxRows];
  const int C = q.n + 1, none = q.R * C, used = none + C;
  const bool dense = used <= kLdsCells;                                   // the same for every lane of the launch
  if (dense)
    for (int k = threadIdx.x; k < used; k += kThreads) cells[k] = 0;
  for (int s = threadIdx.x; s < q.R; s += kThreads)                       // (a shift of a whole side leaves the canvas)
    s_shift[s] = make_int2(max(-q.W, min(q.W, q.shift[2 * s])), max(-q.H, min(q.H, q.shift[2 * s + 1])));
  __syncthreads();
  const bool fast_a = aligned16(q.a), fast_b = aligned16(q.b);
  const unsigned W = (unsigned)q.W, H = (unsigned)q.H;
  PairRun run, cur;                                                       // (row, gathered column); (0, own column)
  auto add = [&](int cell, unsigned cnt) {
    if (dense) atomicAdd(&cells[cell], cnt);
    else atomicAdd(&q.pairs[cell], (int)cnt);
  };
  auto look = [](bool, bool) {};
  auto flush = [&](unsigned cnt) {                                        // a run of row R is counted nowhere
    if (run.a >= q.R) return;
    add(run.a * C + run.b, cnt);
    if (!dense) atomicSub(&q.pairs[none + run.b], (int)cnt);
  };
  auto flush_cur = [&](unsigned cnt) { add(none + cur.b, cnt); };
  for_pieces(q.HW, q.span, [&](long long p0, int valid) {
    int v[kPiece], c[kPiece], zero[kPiece];
    load_ids(q.a, p0, valid, fast_a, v);
    load_bytes<false>(q.b + p0, valid, fast_b, c);
    bool any = false, same = true;
#pragma unroll
    for (int k = 0; k < kPiece; ++k) {
      c[k] = min(c[k], q.n);
      zero[k] = 0;
      any |= k < valid && v[k] < q.R;
      same &= v[k] == v[0];
    }
    walk_pairs(cur, zero, c, valid, look, flush_cur);
    if (!any) {                                                           // no track in the piece: the run ends here
      if (run.cnt) flush(run.cnt);
      run.a = q.R; run.b = 0; run.cnt = 0;
      return;
    }
    const unsigned y = (unsigned)p0 / W, x = (unsigned)p0 - y * W;
    if (same && valid == kPiece && x + kPiece <= W) {
      const int2 d = s_shift[v[0]];
      const unsigned qx = x + (unsigned)d.x, qy = y + (unsigned)d.y;      // a negative position wraps past W and H
      if (qy < H && qx < W && qx + kPiece <= W) {                         // the whole piece lands on one canvas row
        u32x4 w;
        __builtin_memcpy(&w, q.b + ((long long)qy * q.W + qx), sizeof(w));   // 16 bytes at any byte offset
#pragma unroll
        for (int k = 0; k < kPiece; ++k) c[k] = min((int)(w[k >> 2] >> (8 * (k & 3)) & 0xff), q.n);
        walk_pairs(run, v, c, kPiece, look, flush);
        return;
      }
    }
    int last = -1;                                                        // a mixed or clipped piece: a byte per pixel
    int2 d = make_int2(0, 0);
    unsigned xx = x, yy = y;
#pragma unroll
    for (int k = 0; k < kPiece; ++k) {
      int row = q.R, col = 0;
      if (k < valid && v[k] < q.R) {
        if (v[k] != last) { last = v[k]; d = s_shift[last]; }
        const unsigned qx = xx + (unsigned)d.x, qy = yy + (unsigned)d.y;
        if (qx < W && qy < H) { row = v[k]; col = min((int)q.b[(long long)qy * q.W + qx], q.n); }
      }
      v[k] = row; c[k] = col;
      if (++xx == W) { xx = 0; ++yy; }
    }
    walk_pairs(run, v, c, valid, look, flush);
  });
  if (run.cnt) flush(run.cnt);
  if (cur.cnt) flush_cur(cur.cnt);
  if (dense) {
    __syncthreads();
    for (int k = threadIdx.x; k < none; k += kThreads) {                  // row R: area_cur less the rows above
      const unsigned cnt = cells[k];
      if (cnt) atomicSub(&cells[none + k % C], cnt);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < used; k += kThreads) {
      const unsigned cnt = cells[k];                                      // (row R modulo 2^32: it may be negative)
      if (cnt) atomicAdd(&q.pairs[k], (int)cnt);
    }
  }
}

// floor((v * g + 8) / 16) clamped to [-side, side]
__device__ __forceinline__ int predicted_shift(int v, int g, int side) {
  const long long d = ((long long)v * g + 8) >> 4;
  return (int)max((long long)-side, min((long long)side, d));
}

__global__ __launch_bounds__(kSlots) void track_predict_kernel(const int* __restrict__ slots, const int* __restrict__ kin,
                                                               int t, int H, int W, int* __restrict__ shift) {
  const int s = threadIdx.x;
  const int* k = kin + kKinInts * s;
  const bool moving = slots[kSlotInts * s] != 0 && k[5] != 0;
  const int g = t - k[4];
  shift[2 * s] = moving ? predicted_shift(k[2], g, W) : 0;
  shift[2 * s + 1] = moving ? predicted_shift(k[3], g, H) : 0;
}

struct MomentArgs {
  const uint8_t* index;       // [HW]
  unsigned long long* sums;   // [n][3] = {A, Sx, Sy}, zeroed
  long long HW, span;
  int n, W;
};

// {pixels, sum of x, sum of y} of every instance: one run per lane, a counter is touched only when the column changes
__global__ __launch_bounds__(kThreads) void track_moments_kernel(MomentArgs q) {
  __shared__ unsigned long long s_sum[kMaxInst * 3];
  for (int k = threadIdx.x; k < kMaxInst * 3; k += kThreads) s_sum[k] = 0;
  __syncthreads();
  const bool fast = aligned16(q.index);
  const unsigned W = (unsigned)q.W;
  int col = -1;                                                           // the lane's run: an instance or -1 for none
  unsigned area = 0;
  unsigned long long sx = 0, sy = 0;
  auto flush = [&]() {
    if (area) {
      atomicAdd(&s_sum[3 * col], (unsigned long long)area);
      atomicAdd(&s_sum[3 * col + 1], sx);
      atomicAdd(&s_sum[3 * col + 2], sy);
    }
    area = 0; sx = 0; sy = 0;
  };
  for_pieces(q.HW, q.span, [&](long long p0, int valid) {
    int c[kPiece];
    load_bytes<false>(q.index + p0, valid, fast, c);
    bool any = false;
#pragma unroll
    for (int k = 0; k < kPiece; ++k) any |= k < valid && c[k] < q.n;
    if (!any) { flush(); col = -1; return; }
    unsigned y = (unsigned)p0 / W, x = (unsigned)p0 - y * W;
#pragma unroll
    for (int k = 0; k < kPiece; ++k) {
      if (k < valid) {
        const int now = c[k] < q.n ? c[k] : -1;
        if (now != col) { flush(); col = now; }
        if (now >= 0) { ++area; sx += x; sy += y; }
      }
      if (++x == W) { x = 0; ++y; }
    }
  });
  flush();
  __syncthreads();
  for (int k = threadIdx.x; k < 3 * q.n; k += kThreads)
    if (s_sum[k]) atomicAdd(&q.sums[k], s_sum[k]);
}

// floor((32 S + A) / (2 A)): the mean of S / A in 1/16 pixel, half up
__device__ __forceinline__ int centroid16(unsigned long long S, unsigned long long A) {
  return (int)((32 * S + A) / (2 * A));
}

__global__ __launch_bounds__(kSlots) void track_kinematics_kernel(const unsigned long long* __restrict__ sums, int n,
                                                                  const int* __restrict__ inst,
                                                                  const int* __restrict__ slots,
                                                                  const int* __restrict__ status, int t,
                                                                  int* __restrict__ kin) {
  __shared__ int s_kin[kSlots][kKinInts];
  if (status[0]) return;                                                  // the step changed nothing
  const int s = threadIdx.x;
#pragma unroll
  for (int j = 0; j < kKinInts; ++j) s_kin[s][j] = kin[kKinInts * s + j];
  __syncthreads();
  const int slot = s < n ? inst[kInstInts * s] : -1;                      // (one instance per slot: no two lanes meet)
  if (slot >= 0 && slot < kSlots) {
    const bool is_new = inst[kInstInts * s + 4] != 0;
    const unsigned long long A = sums[3 * s];
    int* k = s_kin[slot];
    if (A == 0) {
      if (is_new)
        for (int j = 0; j < kKinInts; ++j) k[j] = 0;
    } else {
      const int cx = centroid16(sums[3 * s + 1], A), cy = centroid16(sums[3 * s + 2], A);
      const int g = t - k[4];
      const bool first = is_new || k[5] == 0 || g <= 0;                   // (g >= 1 for a track seen before)
      const int vx = first ? 0 : (int)(((long long)cx - k[0]) / g), vy = first ? 0 : (int)(((long long)cy - k[1]) / g);
      k[0] = cx; k[1] = cy; k[2] = vx; k[3] = vy; k[4] = t; k[5] = 1;
    }
  }
  __syncthreads();
  const bool free_slot = slots[kSlotInts * s] == 0;
#pragma unroll
  for (int j = 0; j < kKinInts; ++j) kin[kKinInts * s + j] = free_slot ? 0 : s_kin[s][j];
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

extern "C" int cp_map_pairs_shifted(const uint16_t* a, const int32_t* shift, int32_t R, const uint8_t* b, int32_t n,
                                    int32_t H, int32_t W, int32_t* pairs, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && R >= 0 && n >= 0);
  const long long HW = (long long)H * W;
  if (R > kMaxRows || n > kMaxCols || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(a && b && pairs && (R == 0 || shift));
  CP_CHECK_ARG(((uintptr_t)a & 1) == 0 && ((uintptr_t)shift & 3) == 0 && ((uintptr_t)pairs & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int cells = (R + 1) * (n + 1);
  hipLaunchKernelGGL(pairs_clear_kernel, dim3(min((cells + kThreads - 1) / kThreads, kWorkgroups)), dim3(kThreads), 0, st,
                     pairs, cells);
  ShiftArgs q;
  q.a = a; q.shift = shift; q.b = b; q.pairs = pairs; q.HW = HW; q.span = span_for(HW, kWorkgroups);
  q.R = R; q.n = n; q.H = H; q.W = W;
  hipLaunchKernelGGL(map_pairs_shifted_kernel, dim3(span_blocks(HW, q.span)), dim3(kThreads), 0, st, q);
  return cp_launch_status();
}

extern "C" int cp_track_predict(const int32_t* slots, const int32_t* kin, int32_t t, int32_t H, int32_t W, int32_t* shift,
                                void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && t >= 0);
  CP_CHECK_ARG(slots && kin && shift);
  CP_CHECK_ARG(((uintptr_t)slots & 3) == 0 && ((uintptr_t)kin & 3) == 0 && ((uintptr_t)shift & 3) == 0);
  hipLaunchKernelGGL(track_predict_kernel, dim3(1), dim3(kSlots), 0, (hipStream_t)stream, slots, kin, t, H, W, shift);
  return cp_launch_status();
}

extern "C" size_t cp_track_kinematics_workspace_bytes(int32_t n) {
  return n > 0 ? (size_t)n * 3 * sizeof(unsigned long long) : 0;
}

extern "C" int cp_track_kinematics(const uint8_t* index, int32_t n, int32_t H, int32_t W, const int32_t* inst,
                                   const int32_t* slots, const int32_t* status, int32_t t, int32_t* kin, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && n >= 0 && t >= 0);
  const long long HW = (long long)H * W;
  if (n > kMaxInst || HW >= (1LL << 31) || H > kMaxSide || W > kMaxSide) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(index && slots && status && kin && (n == 0 || inst));
  CP_CHECK_ARG(((uintptr_t)inst & 3) == 0 && ((uintptr_t)slots & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
               ((uintptr_t)kin & 3) == 0 && ((uintptr_t)workspace & 7) == 0);
  const size_t need = cp_track_kinematics_workspace_bytes(n);
  if (need && (!workspace || workspace_bytes < need)) return CP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* sums = (unsigned long long*)workspace;
  if (n > 0) {
    if (hipMemsetAsync(sums, 0, need, st) != hipSuccess) return CP_EHIP;
    MomentArgs q;
    q.index = index; q.sums = sums; q.HW = HW; q.span = span_for(HW, 4 * kWorkgroups); q.n = n; q.W = W;
    hipLaunchKernelGGL(track_moments_kernel, dim3(span_blocks(HW, q.span)), dim3(kThreads), 0, st, q);
  }
  hipLaunchKernelGGL(track_kinematics_kernel, dim3(1), dim3(kSlots), 0, st, sums, n, inst, slots, status, t, kin);
  return cp_launch_status();
}
