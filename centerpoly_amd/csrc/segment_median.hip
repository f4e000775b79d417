// Segmented exact medians of a 16-bit image for gfx950: per segment of an id image the pixel count, the number of
// measured pixels (value != 0) and the two middle order statistics of the measured values.  The distance columns of
// the Cityscapes instance-level AP (AP 100 m / AP 50 m) take the median disparity of every ground-truth instance
// from it (datasets/evaluation/distances.py).
//   cp_segment_medians, six launches whatever G and the content, nothing read back in between:
//   (memset)            zeroes the id -> column table and both histogram tables.
//   med_enter_kernel    one workgroup: table[seg_ids[j]] = j + 1 (an id outside 16 bits enters nothing).
//   med_high_kernel     pass 1 over ids and values, 16 pixels per lane and step, ONE run (column, key) per lane in
//                       registers; key = the value's high byte, 256 for "no measurement", and a pixel of no segment is
//                       the run (0, 0) whatever its value.  Disparity is smooth inside an instance, so a run mostly ends
//                       with the instance.  A counter is touched only when the run ends.
//   med_pick_kernel     one wave per segment: pixels, valid, and for both ranks (valid - 1) / 2 and valid / 2 the high
//                       byte that holds them and the rank that is left inside it.  The two may differ.
//   med_low_kernel      pass 2, the same walk: the low-byte histogram of the at most two picked high bytes per segment;
//                       every other pixel is the run (0, 0).
//   med_value_kernel    one wave per segment: the low bytes of both ranks, v_lo and v_hi.
// Both passes have two regimes, chosen from G: the workgroup's table in LDS where it fits (G <= 59 in pass 1, G <= 30
// in pass 2; a street scene), its non-zero cells flushed with one global atomic each; straight global atomics
// otherwise, which with that many segments spread over many cells.
// Integer atomics only: the counts do not depend on the order of the additions.
// The piece, span and run scheme, the loaders and the run walker are pixel_pieces.h's.
#include "pixel_pieces.h"

namespace {

constexpr int kMaxSeg = 1024;
constexpr int kWorkgroups = 256;                        // one per CU
constexpr int kLdsCells = 15360;                        // 60 KB of counters per workgroup
constexpr int kKeys = 257;                              // pass 1: 256 high bytes, then "no measurement"
constexpr int kNoValue = 256;
constexpr int kLow = 256, kSlots = 2;                   // pass 2: per segment two tables of low bytes

struct MedianArgs {
  const uint16_t* ids;        // [HW]
  const uint16_t* values;     // [HW]
  const uint16_t* table;      // [65536]: column + 1, 0 for no segment
  int* high;                  // [G][kKeys]
  int4* pick;                 // [G]: high byte of rank lo, rank inside it, high byte of rank hi, rank inside it
  int* low;                   // [G][kSlots][kLow]
  long long HW, span;         // pixels, pixels per workgroup (a multiple of kTile)
  int G;
};

__global__ __launch_bounds__(kMaxSeg) void med_enter_kernel(const int* __restrict__ seg_ids, int G,
                                                            uint16_t* __restrict__ table) {
  const int t = threadIdx.x;
  if (t < G && seg_ids[t] >= 0 && seg_ids[t] < kIds) table[seg_ids[t]] = (uint16_t)(t + 1);
}

// the piece's ids -> columns + 1 in place (the padding repeats the entry before it)
__device__ __forceinline__ void to_columns(const uint16_t* __restrict__ table, int (&c)[kPiece]) {
  int prev_id = c[0], prev_col = table[prev_id];
  c[0] = prev_col;
#pragma unroll
  for (int k = 1; k < kPiece; ++k) {
    if (c[k] != prev_id) { prev_id = c[k]; prev_col = table[prev_id]; }
    c[k] = prev_col;
  }
}

// The walk of both passes over the workgroup's span.  key(col, value, k) turns pixel k of a piece into the run's
// pair (a, b), a == 0 for a pixel that is not counted; a run of `cnt` pixels lands in cell (a - 1) * width + b of
// `global`, through the workgroup's LDS table when all `used` cells fit.
template <typename Key>
__device__ __forceinline__ void walk_counted(const MedianArgs& a, int* __restrict__ global, int width, int used,
                                             unsigned* cells, Key key) {
  const bool dense = used <= kLdsCells;                                   // the same for every lane of the launch
  if (dense) {
    for (int k = threadIdx.x; k < used; k += kThreads) cells[k] = 0;
    __syncthreads();
  }
  const bool fast_ids = aligned16(a.ids), fast_values = aligned16(a.values);
  PairRun run;
  auto look = [](bool, bool) {};
  auto flush = [&](unsigned cnt) {
    if (run.a == 0) return;
    const int cell = (run.a - 1) * width + run.b;
    if (dense) atomicAdd(&cells[cell], cnt);
    else atomicAdd(&global[cell], (int)cnt);
  };
  for_pieces(a.HW, a.span, [&](long long p0, int valid) {
    int c[kPiece], v[kPiece];
    load_ids(a.ids, p0, valid, fast_ids, c);
    load_ids(a.values, p0, valid, fast_values, v);
    to_columns(a.table, c);
    key(c, v);
    walk_pairs(run, c, v, valid, look, flush);
  });
  if (run.cnt) flush(run.cnt);
  if (dense) {
    __syncthreads();
    for (int k = threadIdx.x; k < used; k += kThreads) {
      const unsigned cnt = cells[k];
      if (cnt) atomicAdd(&global[k], (int)cnt);
    }
  }
}

__global__ __launch_bounds__(kThreads) void med_high_kernel(MedianArgs a) {
  __shared__ unsigned cells[kLdsCells];
  walk_counted(a, a.high, kKeys, a.G * kKeys, cells, [](int (&c)[kPiece], int (&v)[kPiece]) {
#pragma unroll
    for (int k = 0; k < kPiece; ++k) v[k] = c[k] ? (v[k] ? v[k] >> 8 : kNoValue) : 0;
  });
}

__global__ __launch_bounds__(kThreads) void med_low_kernel(MedianArgs a) {
  __shared__ unsigned cells[kLdsCells];
  int col = 0, b_lo = -1, b_hi = -1;                                      // the picked high bytes of the lane's column
  walk_counted(a, a.low, kLow, a.G * kSlots * kLow, cells, [&](int (&c)[kPiece], int (&v)[kPiece]) {
#pragma unroll
    for (int k = 0; k < kPiece; ++k) {
      if (c[k] != col) {
        col = c[k];
        b_lo = b_hi = -1;
        if (col) { const int4 p = a.pick[col - 1]; b_lo = p.x; b_hi = p.z; }
      }
      int slot = 0;                                                       // 1 + kSlots * column + which table
      if (col && v[k]) {
        const int hi = v[k] >> 8;
        if (hi == b_lo) slot = kSlots * col - 1;
        else if (hi == b_hi) slot = kSlots * col;
      }
      c[k] = slot;
      v[k] = slot ? v[k] & 0xff : 0;
    }
  });
}

// This lane holds bins 4 * lane .. 4 * lane + 3 of a 256-bin histogram.  The bin that holds the 0-based ascending
// rank r (r < the histogram's total), and in `inside` the rank that is left within that bin; the same on every lane.
__device__ __forceinline__ int wave_rank_bin(const int (&c)[4], int r, int& inside) {
  const int lane = threadIdx.x & (CP_WAVE - 1);
  const int own = c[0] + c[1] + c[2] + c[3];
  int inc = own;                                                          // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const int x = __shfl_up(inc, o, CP_WAVE);
    if (lane >= o) inc += x;
  }
  const unsigned long long has = __ballot(r < inc);
  const int src = has ? __ffsll((long long)has) - 1 : CP_WAVE - 1;
  int bin = 4 * lane, left = r - (inc - own);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (bin == 4 * lane + k && left >= c[k]) { left -= c[k]; ++bin; }
  inside = __shfl(left, src, CP_WAVE);
  return __shfl(bin, src, CP_WAVE);
}

__global__ __launch_bounds__(CP_WAVE) void med_pick_kernel(const int* __restrict__ high, int4* __restrict__ pick,
                                                           int* __restrict__ out) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const int* h = high + (long long)j * kKeys;
  const int c[4] = {h[4 * lane], h[4 * lane + 1], h[4 * lane + 2], h[4 * lane + 3]};
  int valid = c[0] + c[1] + c[2] + c[3];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) valid += __shfl_xor(valid, o, CP_WAVE);
  int4 p = make_int4(-1, 0, -1, 0);
  if (valid > 0) {                                                        // the same on every lane
    p.x = wave_rank_bin(c, (valid - 1) / 2, p.y);
    p.z = wave_rank_bin(c, valid / 2, p.w);
  }
  if (lane == 0) {
    pick[j] = p;
    out[4 * j] = valid + h[kNoValue];
    out[4 * j + 1] = valid;
    if (valid == 0) { out[4 * j + 2] = 0; out[4 * j + 3] = 0; }
  }
}

__global__ __launch_bounds__(CP_WAVE) void med_value_kernel(const int* __restrict__ low, const int4* __restrict__ pick,
                                                            int* __restrict__ out) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const int4 p = pick[j];
  if (p.x < 0) return;                                                    // no measured pixel: written by the pick
  const int* t0 = low + (long long)j * kSlots * kLow;
  const int* t1 = p.z == p.x ? t0 : t0 + kLow;                            // both ranks in one high byte: one table
  const int c0[4] = {t0[4 * lane], t0[4 * lane + 1], t0[4 * lane + 2], t0[4 * lane + 3]};
  const int c1[4] = {t1[4 * lane], t1[4 * lane + 1], t1[4 * lane + 2], t1[4 * lane + 3]};
  int unused;
  const int lo = wave_rank_bin(c0, p.y, unused), hi = wave_rank_bin(c1, p.w, unused);
  if (lane == 0) {
    out[4 * j + 2] = p.x << 8 | lo;
    out[4 * j + 3] = p.z << 8 | hi;
  }
}

// the workspace: the id -> column table, then the three tables of ints
constexpr size_t kTableBytes = (size_t)kIds * sizeof(uint16_t);
static inline size_t pick_offset(int G) { return kTableBytes + cp_align_up((size_t)G * kKeys * sizeof(int), 16); }
static inline size_t low_offset(int G) { return pick_offset(G) + (size_t)G * sizeof(int4); }

}  // namespace

extern "C" size_t cp_segment_medians_workspace_bytes(int32_t G, int32_t H, int32_t W) {
  (void)H; (void)W;
  if (G < 0 || G > kMaxSeg) return 0;
  return low_offset(G) + (size_t)G * kSlots * kLow * sizeof(int);
}

extern "C" int cp_segment_medians(const uint16_t* ids, const uint16_t* values, int32_t H, int32_t W,
                                  const int32_t* seg_ids, int32_t G, int32_t* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(G >= 0 && H > 0 && W > 0);
  const long long HW = (long long)H * W;
  if (G > kMaxSeg || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  if (G == 0) return CP_OK;
  const size_t need = cp_segment_medians_workspace_bytes(G, H, W);
  if (!workspace || workspace_bytes < need) return CP_EWORKSPACE;
  CP_CHECK_ARG(ids && values && seg_ids && out);
  CP_CHECK_ARG(((uintptr_t)ids & 1) == 0 && ((uintptr_t)values & 1) == 0 && ((uintptr_t)seg_ids & 3) == 0 &&
               ((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  MedianArgs a;
  a.ids = ids; a.values = values; a.table = (const uint16_t*)ws; a.high = (int*)(ws + kTableBytes);
  a.pick = (int4*)(ws + pick_offset(G)); a.low = (int*)(ws + low_offset(G));
  a.HW = HW; a.span = span_for(HW, kWorkgroups); a.G = G;
  (void)hipMemsetAsync(workspace, 0, need, st);
  hipLaunchKernelGGL(med_enter_kernel, dim3(1), dim3(kMaxSeg), 0, st, seg_ids, G, (uint16_t*)ws);
  const unsigned blocks = span_blocks(HW, a.span);
  hipLaunchKernelGGL(med_high_kernel, dim3(blocks), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(med_pick_kernel, dim3(G), dim3(CP_WAVE), 0, st, a.high, a.pick, out);
  hipLaunchKernelGGL(med_low_kernel, dim3(blocks), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(med_value_kernel, dim3(G), dim3(CP_WAVE), 0, st, a.low, a.pick, out);
  return cp_launch_status();
}
