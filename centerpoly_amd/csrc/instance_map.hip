// The instance map of one image for gfx950: up to 128 masks merged, depth resolved, into one map with its
// per-instance tables (cp_instance_map of include/centerpoly_hip.h, where the definitions are).
//
// With torch ops this is an [n, H, W] argmax plus gathers and reductions over every plane.  Here:
//   instance_map_prepare_kernel  one workgroup, eight lanes per instance: liveness, the ordinal k and `value`, the rank
//                                of every live instance with a non-empty clipped box in the `before` order (n <= 128:
//                                a 128 x 128 comparison), the tables in rank order into the workspace, `visible` zeroed
//                                and `box` emptied.
//   instance_map_tile_kernel     a workgroup owns a tile of kTH x kTW pixels, a lane a piece of 16 pixels of one row.
//                                The workgroup bins the ranked boxes against its tile into an LDS list that keeps the
//                                rank order (two wave ballots), so a lane walks the list front to back, reads a plane
//                                only where the piece meets the box and is not yet decided, and the first cover wins.
//                                Pixel masks are 16-bit words, the winners of a piece four words of rank bytes.  Counts
//                                and boxes go run by run (a whole wave at once where its 1024 pixels have one winner)
//                                into LDS tables in rank order, and from there, once per workgroup and instance, into
//                                global memory with integer atomics.
// Two launches, whatever n is.  Integer atomics only: the result does not depend on the order of the additions.
#include <limits.h>

#include "pixel_pieces.h"                               // the piece and its byte loader

namespace {

constexpr int kMaxInst = 128;
constexpr int kTW = 256, kTH = 16;                      // the tile: 16 pieces across, one row per 16 lanes
constexpr int kBatch = 8;                               // planes a lane loads before it resolves them
constexpr int kNone = 255;                              // no winner (rank byte and index value)
static_assert(kTW / kPiece * kTH == kThreads, "one piece per lane");

// workspace, int32 words: [0] the number of ranked instances, then the tables in rank order
constexpr int kWsIdx = 4, kWsVal = kWsIdx + kMaxInst, kWsLab = kWsVal + kMaxInst, kWsBox = kWsLab + kMaxInst;
constexpr int kWsWords = kWsBox + 4 * kMaxInst;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// before(i, j) of the header for two priorities (has_prio == false: the index alone)
__device__ __forceinline__ bool before(bool has_prio, float pi, int i, float pj, int j) {
  if (!has_prio) return i < j;
  const bool ni = pi != pi, nj = pj != pj;
  if (ni || nj) return ni == nj ? i < j : nj;            // a NaN sorts after every number
  return pi < pj || (pi == pj && i < j);
}

// kParts lanes per instance, each comparing it with a slice of the others (one lane per instance walks 128 pairs one
// after the other: tens of microseconds, more than the tile kernel takes with bounds)
constexpr int kParts = 8, kSlice = kMaxInst / kParts;

__global__ __launch_bounds__(kMaxInst * kParts) void instance_map_prepare_kernel(
    int n, int H, int W, const uint8_t* __restrict__ flags, int flag_mask, const int* __restrict__ counts, int min_count,
    const int* __restrict__ label, const float* __restrict__ prio, const int* __restrict__ bounds, int multiplier,
    int* __restrict__ value, int* __restrict__ visible, int* __restrict__ box, int* __restrict__ ws) {
  __shared__ i32x4 s_rec[kMaxInst];                      // label, prio bits, live, ranked: one 16-byte read per pair
  __shared__ int s_k[kMaxInst], s_rank[kMaxInst];
  const int t = threadIdx.x & (kMaxInst - 1), part = threadIdx.x / kMaxInst;
  const bool in = t < n;
  const bool live = in && (flags[t] & flag_mask) != 0 && (!counts || counts[t] > min_count);
  const int lab = in ? label[t] : 0;
  int x0 = 0, y0 = 0, x1 = W - 1, y1 = H - 1;
  if (in && bounds) {
    x0 = max(bounds[4 * t], 0); y0 = max(bounds[4 * t + 1], 0);
    x1 = min(bounds[4 * t + 2], W - 1); y1 = min(bounds[4 * t + 3], H - 1);
  }
  const bool cand = live && x0 <= x1 && y0 <= y1;        // an empty box covers nothing: never ranked
  const float pr = in && prio ? prio[t] : 0.f;
  if (part == 0) {
    s_rec[t] = i32x4{lab, __float_as_int(pr), live, cand};
    s_k[t] = 0;
    s_rank[t] = 0;
  }
  __syncthreads();
  int k = 0, rank = 0;
#pragma unroll
  for (int j = part * kSlice; j < (part + 1) * kSlice; ++j) {   // (slots at and beyond n are neither live nor ranked)
    const i32x4 o = s_rec[j];
    k += j < t && o.z && o.x == lab;
    rank += j != t && o.w && before(prio != nullptr, __int_as_float(o.y), j, pr, t);
  }
  if (k) atomicAdd(&s_k[t], k);
  if (rank) atomicAdd(&s_rank[t], rank);
  const int ranked = __syncthreads_count(part == 0 && cand);
  if (part) return;
  k = s_k[t];
  rank = s_rank[t];
  const int val = live ? (int)((unsigned)lab * (unsigned)multiplier + (unsigned)k) : -1;
  if (in) {
    value[t] = val;
    visible[t] = 0;
    box[4 * t] = W; box[4 * t + 1] = H; box[4 * t + 2] = -1; box[4 * t + 3] = -1;
  }
  if (cand) {
    ws[kWsIdx + rank] = t; ws[kWsVal + rank] = val; ws[kWsLab + rank] = lab;
    ws[kWsBox + 4 * rank] = x0; ws[kWsBox + 4 * rank + 1] = y0;
    ws[kWsBox + 4 * rank + 2] = x1; ws[kWsBox + 4 * rank + 3] = y1;
  }
  if (t == 0) ws[0] = ranked;
}

// bits 7, 15, 23, 31 of nz as bits 0..3 (the products of the four source bits fall on distinct positions: no carry)
__device__ __forceinline__ unsigned pack4(unsigned nz) { return (((nz >> 7) & 0x01010101u) * 0x01020408u) >> 24; }

// bits 0..3 of m as the bytes 0x00 / 0xff of a word (again distinct positions)
__device__ __forceinline__ unsigned spread4(unsigned m) { return (((m & 0xfu) * 0x00204081u) & 0x01010101u) * 0xffu; }

// the 16 mask bytes of one piece as the 16-bit word of its non-zero pixels
__device__ __forceinline__ unsigned cover_bits(u32x4 w) {
  return pack4(nonzero_bytes(w.x)) | pack4(nonzero_bytes(w.y)) << 4 | pack4(nonzero_bytes(w.z)) << 8 |
         pack4(nonzero_bytes(w.w)) << 12;
}

// the pixels k of a piece at column x with x0 <= x + k <= x1, as bits
__device__ __forceinline__ unsigned span_bits(int x, int x0, int x1) {
  const int lo = max(x0 - x, 0), hi = min(x1 - x, kPiece - 1);
  return lo > hi ? 0u : ((2u << hi) - 1u) & ~((1u << lo) - 1u);
}

struct MapArgs {
  const uint8_t* masks;       // [n][HW]
  const int* ws;              // the prepare kernel's tables
  uint8_t* index;             // [HW]
  int* ids;                   // [HW] or null
  int* labels;                // [HW] or null
  int* visible;               // [n]
  int* box;                   // [n][4]
  long long HW;
  int H, W, background;
  unsigned tiles_x;           // tiles across: the grid is one-dimensional (a tall, narrow image has many rows of tiles)
};

// one run of `len` pixels from column x in row y that rank r wins, into the workgroup's tables
__device__ __forceinline__ void add_run(int* cnt, int* bx, int r, int len, int x, int y) {
  atomicAdd(&cnt[r], len);
  atomicMin(&bx[4 * r], x); atomicMin(&bx[4 * r + 1], y);
  atomicMax(&bx[4 * r + 2], x + len - 1); atomicMax(&bx[4 * r + 3], y);
}

__global__ __launch_bounds__(kThreads) void instance_map_tile_kernel(MapArgs a) {
  __shared__ int s_idx[kMaxInst], s_val[kMaxInst], s_lab[kMaxInst], s_box[4 * kMaxInst];
  __shared__ int s_cnt[kMaxInst], s_bx[4 * kMaxInst];
  __shared__ int s_list[kMaxInst];
  __shared__ unsigned long long s_ballot[2];
  const int t = threadIdx.x, lane = t & (CP_WAVE - 1), wave = t >> 6;
  const int tx0 = (int)(blockIdx.x % a.tiles_x) * kTW, ty0 = (int)(blockIdx.x / a.tiles_x) * kTH;
  const int tx1 = min(tx0 + kTW, a.W) - 1, ty1 = min(ty0 + kTH, a.H) - 1;
  const int ranked = a.ws[0];

  // the tables in rank order, and the boxes that meet the tile as a list that keeps the order
  bool hit = false;
  if (t < kMaxInst) {
    s_cnt[t] = 0;
    s_bx[4 * t] = INT_MAX; s_bx[4 * t + 1] = INT_MAX; s_bx[4 * t + 2] = -1; s_bx[4 * t + 3] = -1;
    if (t < ranked) {
      s_idx[t] = a.ws[kWsIdx + t]; s_val[t] = a.ws[kWsVal + t]; s_lab[t] = a.ws[kWsLab + t];
      const int x0 = a.ws[kWsBox + 4 * t], y0 = a.ws[kWsBox + 4 * t + 1];
      const int x1 = a.ws[kWsBox + 4 * t + 2], y1 = a.ws[kWsBox + 4 * t + 3];
      s_box[4 * t] = x0; s_box[4 * t + 1] = y0; s_box[4 * t + 2] = x1; s_box[4 * t + 3] = y1;
      hit = x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
    }
  }
  const unsigned long long votes = __ballot(hit);
  if (wave < 2 && lane == 0) s_ballot[wave] = votes;
  __syncthreads();
  if (hit) s_list[(wave ? __popcll(s_ballot[0]) : 0) + __popcll(votes & ((1ull << lane) - 1ull))] = t;
  const int listed = __popcll(s_ballot[0]) + __popcll(s_ballot[1]);
  __syncthreads();

  // the lane's piece: `valid` pixels from column x of row y
  const int y = ty0 + (t >> 4), x = tx0 + (t & 15) * kPiece;
  const int valid = y < a.H ? max(0, min(kPiece, a.W - x)) : 0;
  const long long p = (long long)y * a.W + x;
  unsigned open = valid ? (2u << (valid - 1)) - 1u : 0u;   // pixels without a winner yet
  unsigned win[4] = {~0u, ~0u, ~0u, ~0u};                  // rank bytes, kNone where nobody covers
  for (int e0 = 0; e0 < listed; e0 += kBatch) {
    u32x4 w[kBatch];
    unsigned span[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {                     // kBatch loads in flight per lane
      w[j] = u32x4{0, 0, 0, 0};
      span[j] = 0;
      if (e0 + j < listed && open) {
        const int r = s_list[e0 + j];
        if (y >= s_box[4 * r + 1] && y <= s_box[4 * r + 3]) span[j] = span_bits(x, s_box[4 * r], s_box[4 * r + 2]) & open;
        if (span[j]) {                                     // (an unaligned row or the row's tail: element loads)
          const uint8_t* mp = a.masks + (long long)s_idx[r] * a.HW + p;
          w[j] = load_bytes<true>(mp, valid, aligned16(mp));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const unsigned got = cover_bits(w[j]) & span[j] & open;
      if (got) {
        const unsigned r4 = (unsigned)s_list[e0 + j] * 0x01010101u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned m = spread4(got >> (4 * q));
          win[q] = (win[q] & ~m) | (r4 & m);
        }
        open &= ~got;
      }
    }
  }

  // the maps
  int r[kPiece];
#pragma unroll
  for (int k = 0; k < kPiece; ++k) r[k] = (win[k >> 2] >> (8 * (k & 3))) & 0xff;
  if (valid) {
    unsigned iw[4] = {0, 0, 0, 0};
    int idv[kPiece], lbv[kPiece];
#pragma unroll
    for (int k = 0; k < kPiece; ++k) {
      const bool some = r[k] != kNone;
      iw[k >> 2] |= (unsigned)(some ? s_idx[r[k]] : kNone) << (8 * (k & 3));
      idv[k] = some ? s_val[r[k]] : a.background;
      lbv[k] = some ? s_lab[r[k]] : a.background;
    }
    if (valid == kPiece && aligned16(a.index + p)) {
      *reinterpret_cast<u32x4*>(a.index + p) = u32x4{iw[0], iw[1], iw[2], iw[3]};
    } else {
#pragma unroll
      for (int k = 0; k < kPiece; ++k)
        if (k < valid) a.index[p + k] = (uint8_t)(iw[k >> 2] >> (8 * (k & 3)));
    }
    if (a.ids) {
      if (valid == kPiece && aligned16(a.ids + p)) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          reinterpret_cast<i32x4*>(a.ids + p)[q] = i32x4{idv[4 * q], idv[4 * q + 1], idv[4 * q + 2], idv[4 * q + 3]};
      } else {
#pragma unroll
        for (int k = 0; k < kPiece; ++k)
          if (k < valid) a.ids[p + k] = idv[k];
      }
    }
    if (a.labels) {
      if (valid == kPiece && aligned16(a.labels + p)) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          reinterpret_cast<i32x4*>(a.labels + p)[q] = i32x4{lbv[4 * q], lbv[4 * q + 1], lbv[4 * q + 2], lbv[4 * q + 3]};
      } else {
#pragma unroll
        for (int k = 0; k < kPiece; ++k)
          if (k < valid) a.labels[p + k] = lbv[k];
      }
    }
  }

  // counts and boxes.  Most waves lie inside one instance or in the background: then the wave adds its pixels up
  // and one lane touches the tables (every lane is here: the votes and shuffles need the whole wave)
  bool one = true;
#pragma unroll
  for (int k = 1; k < kPiece; ++k) one = one && (k >= valid || r[k] == r[0]);
  const unsigned long long have = __ballot(valid > 0);
  if (have) {
    const int r0 = __shfl(r[0], __ffsll((long long)have) - 1, CP_WAVE);
    if (__all(valid == 0 || (one && r[0] == r0))) {
      if (r0 != kNone) {
        int total = valid, lx = valid ? x : INT_MAX, ly = valid ? y : INT_MAX, hx = valid ? x + valid - 1 : -1,
            hy = valid ? y : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          total += __shfl_xor(total, o, CP_WAVE);
          lx = min(lx, __shfl_xor(lx, o, CP_WAVE)); ly = min(ly, __shfl_xor(ly, o, CP_WAVE));
          hx = max(hx, __shfl_xor(hx, o, CP_WAVE)); hy = max(hy, __shfl_xor(hy, o, CP_WAVE));
        }
        if (lane == 0) {
          atomicAdd(&s_cnt[r0], total);
          atomicMin(&s_bx[4 * r0], lx); atomicMin(&s_bx[4 * r0 + 1], ly);
          atomicMax(&s_bx[4 * r0 + 2], hx); atomicMax(&s_bx[4 * r0 + 3], hy);
        }
      }
    } else if (valid) {
      int cur = r[0], start = 0;
#pragma unroll
      for (int k = 1; k < kPiece; ++k) {
        if (k < valid && r[k] != cur) {
          if (cur != kNone) add_run(s_cnt, s_bx, cur, k - start, x + start, y);
          cur = r[k]; start = k;
        }
      }
      if (cur != kNone) add_run(s_cnt, s_bx, cur, valid - start, x + start, y);
    }
  }
  __syncthreads();
  if (t < ranked && s_cnt[t]) {
    const int i = s_idx[t];
    atomicAdd(&a.visible[i], s_cnt[t]);
    atomicMin(&a.box[4 * i], s_bx[4 * t]); atomicMin(&a.box[4 * i + 1], s_bx[4 * t + 1]);
    atomicMax(&a.box[4 * i + 2], s_bx[4 * t + 2]); atomicMax(&a.box[4 * i + 3], s_bx[4 * t + 3]);
  }
}

}  // namespace

extern "C" size_t cp_instance_map_workspace_bytes(int32_t n, int32_t H, int32_t W) {
  (void)n; (void)H; (void)W;
  return (size_t)kWsWords * sizeof(int);                  // the tables in rank order
}

extern "C" int cp_instance_map(const uint8_t* masks, int32_t n, int32_t H, int32_t W, const uint8_t* flags,
                               int32_t flag_mask, const int32_t* counts, int32_t min_count, const int32_t* label,
                               const float* prio, const int32_t* bounds, int32_t multiplier, int32_t background,
                               uint8_t* index, int32_t* ids, int32_t* labels, int32_t* value, int32_t* visible,
                               int32_t* box, void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(n >= 0 && H > 0 && W > 0 && multiplier >= 1);
  const long long HW = (long long)H * W;
  if (n > kMaxInst || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(index && (n == 0 || (masks && flags && label && value && visible && box)));
  if (!workspace || workspace_bytes < cp_instance_map_workspace_bytes(n, H, W)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)ids & 3) == 0 && ((uintptr_t)labels & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  int* ws = (int*)workspace;
  hipLaunchKernelGGL(instance_map_prepare_kernel, dim3(1), dim3(kMaxInst * kParts), 0, st, n, H, W, flags, flag_mask, counts,
                     min_count, label, prio, bounds, multiplier, value, visible, box, ws);
  MapArgs a;
  a.masks = masks; a.ws = ws; a.index = index; a.ids = ids; a.labels = labels; a.visible = visible; a.box = box;
  a.HW = HW; a.H = H; a.W = W; a.background = background;
  a.tiles_x = (unsigned)((W + kTW - 1) / kTW);
  const unsigned tiles_y = (unsigned)((H + kTH - 1) / kTH);                 // H * W < 2^31: fewer than 2^27 tiles
  hipLaunchKernelGGL(instance_map_tile_kernel, dim3(a.tiles_x * tiles_y), dim3(kThreads), 0, st, a);
  return cp_launch_status();
}
