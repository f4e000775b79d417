// The piece reader shared by the kernels that stream a 16-bit id image beside byte images (instance_eval.hip,
// instance_map.hip, pixel_eval.hip, panoptic.hip).  A workgroup of 256 lanes owns a span of whole tiles; per step a
// lane takes one PIECE, 16 consecutive pixels: 16-byte loads where the buffer is aligned and the piece is whole,
// element loads for an unaligned buffer or the span's tail.  Runs of equal values are collapsed in registers before
// any counter is touched.  Device and host inline code only.
#pragma once
#include "cp_common.h"

constexpr int kThreads = 256;
constexpr int kPiece = 16;                              // pixels per lane and step
constexpr int kTile = kThreads * kPiece;                // pixels per workgroup and step
constexpr int kIds = 65536;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// bit 8j + 7 of the result is set where byte j of w is non-zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
  return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
}

// The 16 ids of the piece at p0, of which the first `valid` lie inside the span; `fast`: `ids` is 16-byte aligned.
// The padding contract: an entry at or past `valid` repeats the id before it (0 when valid == 0), so it never
// starts a run; a caller that counts pixels masks them out with k < valid.
__device__ __forceinline__ void load_ids(const uint16_t* ids, long long p0, int valid, bool fast, int (&v)[kPiece]) {
  if (fast && valid == kPiece) {
    const uint4 a = *reinterpret_cast<const uint4*>(ids + p0), b = *reinterpret_cast<const uint4*>(ids + p0 + 8);
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[2 * k] = w[k] & 0xffff; v[2 * k + 1] = w[k] >> 16; }
  } else {
#pragma unroll
    for (int k = 0; k < kPiece; ++k) v[k] = k < valid ? ids[p0 + k] : (k ? v[k - 1] : 0);
  }
}

// The 16 bytes of the piece at p as four words, bytes at and past `valid` read as zero; `fast`: p is 16-byte
// aligned.  kStream: a non-temporal load, for planes that are read once.
template <bool kStream>
__device__ __forceinline__ u32x4 load_bytes(const uint8_t* p, int valid, bool fast) {
  if (fast && valid == kPiece) {
    if (kStream) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return *reinterpret_cast<const u32x4*>(p);
  }
  unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kPiece; ++k)
    if (k < valid) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
  return u32x4{w[0], w[1], w[2], w[3]};
}

// the same bytes, one per int
template <bool kStream>
__device__ __forceinline__ void load_bytes(const uint8_t* p, int valid, bool fast, int (&q)[kPiece]) {
  if (fast && valid == kPiece) {
    const u32x4 w = load_bytes<kStream>(p, kPiece, true);
#pragma unroll
    for (int k = 0; k < kPiece; ++k) q[k] = w[k >> 2] >> (8 * (k & 3)) & 0xff;
  } else {
#pragma unroll
    for (int k = 0; k < kPiece; ++k) q[k] = k < valid ? p[k] : 0;
  }
}

// pixels per workgroup: whole tiles, about `want` workgroups over the image; and the workgroups that makes
static inline long long span_for(long long HW, long long want) {
  const long long tiles = (HW + kTile - 1) / kTile;
  return (tiles + want - 1) / want * kTile;
}
static inline unsigned span_blocks(long long HW, long long span) { return (unsigned)((HW + span - 1) / span); }

// body(p0, valid) for every piece of this lane in its workgroup's span, valid > 0.  A lane leaves at the span's end:
// for kernels without wave-wide operations (the others walk on with valid == 0 and keep their own loop).
template <typename Body>
__device__ __forceinline__ void for_pieces(long long HW, long long span, Body body) {
  const long long begin = (long long)blockIdx.x * span, end = min(begin + span, HW);
  for (long long t0 = begin; t0 < end; t0 += kTile) {
    const long long p0 = t0 + (long long)threadIdx.x * kPiece;
    const int valid = (int)min((long long)kPiece, end - p0);
    if (valid <= 0) break;
    body(p0, valid);
  }
}

// The ONE run a lane keeps in registers across all its steps: `cnt` pixels so far of the pair (a, b).
struct PairRun {
  int a = -1, b = -1;
  unsigned cnt = 0;
};

// One piece into the run.  Where the pair changes: flush(cnt) of the run that ends (run.a, run.b still its pair),
// then look(a_changed, b_changed) with the new pair in place, so that only the half that changed is looked up.  The
// last run stays open: the caller flushes it once after its loop.
template <typename Look, typename Flush>
__device__ __forceinline__ void walk_pairs(PairRun& run, const int (&a)[kPiece], const int (&b)[kPiece], int valid,
                                           Look look, Flush flush) {
#pragma unroll
  for (int k = 0; k < kPiece; ++k) {
    if (k < valid) {
      const bool da = a[k] != run.a, db = b[k] != run.b;
      if (da || db) {
        if (run.cnt) flush(run.cnt);
        run.a = a[k]; run.b = b[k]; run.cnt = 0;
        look(da, db);
      }
      ++run.cnt;
    }
  }
}
