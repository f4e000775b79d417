// What the device merges of detection rows share (merge_nms.hip: the literal merge; mask_nms.hip: the mask merge), and
// the only place where it is written: the order of the arg-max, the class of a row, the stable partition by class and
// merge_outputs' cut.  The selection between the partition and the cut is each merge's own.  Device inline code only.
#pragma once
#include <type_traits>

#include "cp_common.h"

namespace row_merge {

constexpr int kThreads = 1024;                                            // the workgroup of class_partition and cut_rows
constexpr int kWaves = kThreads / CP_WAVE;

// LDS writes of some lanes become visible to the other lanes of the same wave (which runs in lock-step: no barrier)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A score and its position in one word whose order is the arg-max's: a higher score wins, then the lower position
// (-0 and +0 are equal scores).  Every key of a position is above 0, the key of "nothing".
__device__ __forceinline__ unsigned long long score_key(float s, int pos) {
  if (s == 0.f) s = 0.f;
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (0xffffffffu - (unsigned)pos);
}

// the largest key of the 64 lanes, in every lane: DPP row shifts and row broadcasts (a lane without a source keeps its
// own key, and max is idempotent), the result read from lane 63.  All 64 lanes are active where this is called.
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned long long max_key_dpp(unsigned long long k) {
  const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWS, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWS, 0xf, false);
  const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
  return o > k ? o : k;
}

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k) {
  k = max_key_dpp<0x111, 0xf>(k);                                         // row_shr:1
  k = max_key_dpp<0x112, 0xf>(k);                                         // row_shr:2
  k = max_key_dpp<0x114, 0xf>(k);                                         // row_shr:4
  k = max_key_dpp<0x118, 0xf>(k);                                         // row_shr:8: lane 15 of a row holds the row's
  k = max_key_dpp<0x142, 0xa>(k);                                         // row_bcast:15 into rows 1, 3: lanes 31, 63 two rows'
  k = max_key_dpp<0x143, 0xc>(k);                                         // row_bcast:31 into rows 2, 3: lane 63 all four
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// the class of a row as `cls == j` of the numpy split sees it: -1 when no j of [0, C) equals it
__device__ __forceinline__ int class_of(float c, int C) {
  const int ci = (c >= 0.f && c < (float)C) ? (int)c : -1;
  return ci >= 0 && (float)ci == c ? ci : -1;
}

// The stable partition by class of n rows, by every thread of a workgroup of kThreads.  The caller has stored the rows'
// classes in cls[0, n) (LDS; class_of, so below 128) and syncs nothing; rank, cnt and start are its LDS too, of n rows
// and C classes.  On return rank[r] is the position of row r within its class and start[j] the first slot of class j:
// row r of class ci >= 0 belongs at start[ci] + rank[r], which the caller scatters to.  seg_start and seg_len [C]
// (memory) receive the table.
__device__ __forceinline__ void class_partition(const signed char* cls, unsigned short* rank, int* cnt, int* start,
                                                int n, int C, int* seg_start, int* seg_len) {
  const int t = threadIdx.x, lane = t & (CP_WAVE - 1), wave = t / CP_WAVE;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int j = wave; j < C; j += kWaves) {                                // one wave per class in turn: the order is fixed
    int run = 0;
    for (int r0 = 0; r0 < n; r0 += CP_WAVE) {
      const int r = r0 + lane;
      const bool mine = r < n && cls[r] == j;
      const unsigned long long m = __ballot(mine);
      if (mine) rank[r] = (unsigned short)(run + __popcll(m & below));
      run += __popcll(m);
    }
    if (lane == 0) cnt[j] = run;
  }
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int j = 0; j < C; ++j) {
      start[j] = acc;
      seg_start[j] = acc;
      seg_len[j] = cnt[j];
      acc += cnt[j];
    }
  }
  __syncthreads();
}

// the LDS of cut_rows for up to kRowsPerThread * kThreads slots
template <int kRowsPerThread>
struct CutLds {
  alignas(16) float score[kRowsPerThread * kThreads];                     // (the rank count reads four at a time)
  int excl[kRowsPerThread * kThreads + 1];                                // kept rows before slot r
  int wave[kWaves];
  float thresh;
};

// `holds` of a table without gaps: the rows are as many as the slots, and no barrier has to count them
struct EverySlot {
  __device__ bool operator()(int) const { return true; }
};

// merge_outputs' cut, by every thread of a workgroup of kThreads, on slots [0, n), n <= kRowsPerThread * kThreads, that
// lie class by class as the segment table says: with more rows than max_per_image, the rows whose score is >= the
// (rows - max_per_image)-th smallest (np.partition(scores, kth)[kth] by rank counting; ties at the threshold stay).
//   holds(r)  whether slot r holds a row (a value the caller made visible to the whole workgroup)
//   score(r)  its score        row(r)  where its source row lies; both asked of slots that hold a row only
// Writes counts[0], the kept rows; counts[1 + c] of every class from the segment table, clamped to the slots; and the
// kept rows to `out` in slot order, the slot's score in column 4.
template <int kRowsPerThread, class Holds, class Score, class Row>
__device__ __forceinline__ void cut_rows(CutLds<kRowsPerThread>& s, int n, Holds holds, Score score, Row row,
                                         const int* seg_start, const int* seg_len, int C, int max_per_image, int ncols,
                                         float* out, int* counts) {
  constexpr bool kEvery = std::is_same<Holds, EverySlot>::value;
  const int t = threadIdx.x, lane = t & (CP_WAVE - 1), wave = t / CP_WAVE;
  if (t == 0) { s.thresh = -__builtin_inff(); s.excl[0] = 0; }
  int total = 0;                                                          // the rows
  for (int r0 = 0; r0 < n; r0 += kThreads) {
    const int r = r0 + t;
    const bool has = r < n && holds(r);
    if (r < n) s.score[r] = has ? score(r) : __builtin_inff();            // an empty slot counts below no score
    if constexpr (!kEvery) total += __syncthreads_count(has);
  }
  if constexpr (kEvery) {
    total = n;
    __syncthreads();
  }
  const bool cut = total > max_per_image;
  if (cut) {                                                              // np.partition(scores, kth)[kth]
    const int kth = total - max_per_image;
    for (int r = t; r < n; r += kThreads) {
      if (!holds(r)) continue;
      const float v = s.score[r];
      int lt = 0, le = 0;
      for (int j = 0; j < n; ++j) {                                       // every lane reads the same address
        const float w = s.score[j];
        lt += w < v ? 1 : 0;
        le += w <= v ? 1 : 0;
      }
      if (lt <= kth && kth < le) s.thresh = v;                            // ties write the same value
    }
  }
  __syncthreads();
  const float thresh = s.thresh;
  // keep flags of slots kRowsPerThread * t .. and their prefix sum over the workgroup
  int keep[kRowsPerThread], mine = 0;
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    const int r = kRowsPerThread * t + q;
    keep[q] = r < n && holds(r) && (!cut || s.score[r] >= thresh) ? 1 : 0;
    mine += keep[q];
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const int up = __shfl_up(incl, o, CP_WAVE);
    if (lane >= o) incl += up;
  }
  if (lane == CP_WAVE - 1) s.wave[wave] = incl;
  __syncthreads();
  int before = incl - mine;
  for (int w = 0; w < wave; ++w) before += s.wave[w];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    before += keep[q];
    s.excl[kRowsPerThread * t + q + 1] = before;
  }
  __syncthreads();
  if (t == 0) counts[0] = s.excl[n];
  if (t < C) {
    int s0 = seg_start[t], s1 = s0 + seg_len[t];
    s0 = s0 < 0 ? 0 : (s0 > n ? n : s0);
    s1 = s1 < s0 ? s0 : (s1 > n ? n : s1);
    counts[1 + t] = s.excl[s1] - s.excl[s0];
  }
  const long long cells = (long long)n * ncols;
  for (long long e = t; e < cells; e += kThreads) {
    const int r = (int)(e / ncols), d = s.excl[r];
    const long long c = e - (long long)r * ncols;                         // (64 bits: row(r) + c folds to table + e)
    if (s.excl[r + 1] != d) {
      const float own = row(r)[c], sc = s.score[r];                       // two loads, not one from either address space
      out[(long long)d * ncols + c] = c == 4 ? sc : own;
    }
  }
}

}  // namespace row_merge
