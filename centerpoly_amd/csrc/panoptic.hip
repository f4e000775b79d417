// Panoptic quality (the protocol of evalPanopticSemanticLabeling's pq_compute_single_core, with the ground-truth
// segments createPanopticImgs derives from the instance-id image) for gfx950, counted AND matched on the device: no
// value comes back to the host per image.
//   cp_panoptic_pairs, five launches whatever the content:
//   pan_clear_kernel     zeroes the presence bytes and the pair table.
//   pan_presence_kernel  one pass over the ids: presence[v] = 1.  A lane keeps its last value in a register and stores
//                        only when it changes (all writers store the same byte, so the race is harmless).
//   pan_compact_kernel   ONE workgroup of 1024 lanes, 64 ids each: which present values are segments (label evaluated),
//                        a block scan of their number, then the table id -> row (0 VOID, 1 .. 1024, 0xffff for a
//                        segment past the 1024th) and the rows {value, label, crowd, 0} of `seg`, ascending by value.
//   pan_count_kernel     the hot path: one workgroup per CU over a span of pixels, 16 pixels per lane and step, ONE run
//                        (id, column, count) per lane in registers; a counter is touched only when the pair changes.
//                        Two regimes, chosen in the kernel from G (the host never learns G):
//                          dense   (min(G, 1024) + 1) * (n + 1) <= kLdsCells (15360 cells, 60 KB of the CU's 160 KB):
//                                  the workgroup's table lives in LDS; at the end its non-zero cells go to the global
//                                  table, one atomic per cell and workgroup.  A street scene (tens x tens) is here.
//                          sparse  otherwise (up to 1025 x 256 cells, 1 MB: no LDS holds it): every run goes straight
//                                  to the global table, which stays in L2.  With that many segments runs are short but
//                                  spread over many cells, so the atomics seldom meet.
//   pan_area_kernel      one wave per row: seg[r][3] = sum of the row (seg[0][1] for VOID).  No second atomic per run.
//   cp_panoptic_match, one launch of one workgroup: ONE coalesced pass over the pair table gives the column areas and
//   per row its only candidate (2 inter > union needs 2 inter > area_g); then existing slots, crowd rows, the matches
//   (at most one per row and per column, so no two lanes write the same entry), and one lane per label adds the
//   matched IoUs in ascending row order onto the running float64 sum -- the order of the evaluator's loop.
// Integer atomics only in the counting: the counts do not depend on the order of the additions.  The float64 sum is
// divisions and additions, nothing a contraction could fuse.
// The piece, span and run scheme, the loaders and the run walker are pixel_pieces.h's.
#include "pixel_pieces.h"

namespace {

constexpr int kMaxLabels = 64, kMaxRows = 1024, kMaxSlots = 255;
constexpr int kWorkgroups = 256;                        // one per CU
constexpr int kLdsCells = 15360;                        // dense regime: 60 KB of counters per workgroup
constexpr unsigned kDropped = 0xffff;                   // id -> row: a segment past the 1024th
constexpr int kOneThreads = 1024;                       // the two single-workgroup kernels

struct LabelFlags {
  uint8_t f[kMaxLabels];                                // bit 0 evaluated, bit 1 has instances; 0 from L on
};

struct MatchTables {
  int16_t pred_label[256];                              // label of a slot, -1 outside [0, L)
  uint8_t flags[kMaxLabels];
};

__global__ __launch_bounds__(kThreads) void pan_clear_kernel(unsigned* __restrict__ presence_words,
                                                             int* __restrict__ pairs, int cells) {
  const int stride = gridDim.x * kThreads, first = blockIdx.x * kThreads + threadIdx.x;
  for (int k = first; k < kIds / 4; k += stride) presence_words[k] = 0;
  for (int k = first; k < cells; k += stride) pairs[k] = 0;
}

__global__ __launch_bounds__(kThreads) void pan_presence_kernel(const uint16_t* __restrict__ ids, long long HW,
                                                                long long span, uint8_t* __restrict__ presence) {
  const bool fast = aligned16(ids);
  int last = -1;
  // (for_pieces' loop, written out: through the lambda the compiler no longer splits the whole pieces, which need no
  // k < valid, from the tail)
  const long long begin = (long long)blockIdx.x * span, end = min(begin + span, HW);
  for (long long t0 = begin; t0 < end; t0 += kTile) {
    const long long p0 = t0 + (long long)threadIdx.x * kPiece;
    const int valid = (int)min((long long)kPiece, end - p0);
    if (valid <= 0) break;
    int v[kPiece];
    load_ids(ids, p0, valid, fast, v);
#pragma unroll
    for (int k = 0; k < kPiece; ++k)
      if (k < valid && v[k] != last) { last = v[k]; presence[last] = 1; }
  }
}

__global__ __launch_bounds__(kOneThreads) void pan_compact_kernel(LabelFlags fl, const uint8_t* __restrict__ presence,
                                                                  int id_divisor, int id_direct_below, int L,
                                                                  uint16_t* __restrict__ rowtab, int* __restrict__ seg) {
  __shared__ int wave_total[kOneThreads / CP_WAVE];
  __shared__ uint8_t s_flags[kMaxLabels];
  const int t = threadIdx.x, lane = t & (CP_WAVE - 1), wave = t / CP_WAVE, first = t * 64;
  if (t < kMaxLabels) s_flags[t] = t < L ? fl.f[t] : 0;
  __syncthreads();
  unsigned long long bits = 0;                                           // which of this lane's 64 ids are segments
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 w4 = *reinterpret_cast<const uint4*>(presence + first + 16 * q);
    const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (w[k >> 2] >> (8 * (k & 3)) & 0xff) {
        const int v = first + 16 * q + k;
        const int g = v < id_direct_below ? v : v / id_divisor;
        if (g < L && (s_flags[g] & 1)) bits |= 1ull << (16 * q + k);
      }
    }
  }
  const int count = __popcll(bits);
  int inc = count;                                                        // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const int x = __shfl_up(inc, o, CP_WAVE);
    if (lane >= o) inc += x;
  }
  if (lane == CP_WAVE - 1) wave_total[wave] = inc;
  __syncthreads();
  int before = 0, G = 0;
  for (int k = 0; k < kOneThreads / CP_WAVE; ++k) {
    if (k < wave) before += wave_total[k];
    G += wave_total[k];
  }
  int row = before + inc - count + 1;
  for (int q = 0; q < 8; ++q) {                                           // 8 ids per 16-byte store
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (bits >> (8 * q + k) & 1) {
        unsigned r = kDropped;
        if (row <= kMaxRows) {
          const int v = first + 8 * q + k;
          const int g = v < id_direct_below ? v : v / id_divisor;
          r = (unsigned)row;
          *reinterpret_cast<int4*>(seg + 4 * row) =
              make_int4(v, g, v < id_direct_below && (s_flags[g] & 2) ? 1 : 0, 0);
        }
        ++row;
        w[k >> 1] |= r << (16 * (k & 1));
      }
    }
    *reinterpret_cast<uint4*>(rowtab + first + 8 * q) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (t == 0) *reinterpret_cast<int4*>(seg) = make_int4(G, 0, 0, 0);
}

struct CountArgs {
  const uint8_t* index;       // [HW]
  const uint16_t* ids;        // [HW]
  const uint16_t* rowtab;     // [65536]
  const int* seg;             // seg[0] = G
  int* pairs;                 // [1025][n + 1]
  long long HW, span;         // pixels, pixels per workgroup (a multiple of kTile)
  int n;
};

__global__ __launch_bounds__(kThreads) void pan_count_kernel(CountArgs a) {
  __shared__ unsigned cells[kLdsCells];
  const int C = a.n + 1, used = (min(a.seg[0], kMaxRows) + 1) * C;
  const bool dense = used <= kLdsCells;                                   // the same for every lane of the launch
  if (dense) {
    for (int k = threadIdx.x; k < used; k += kThreads) cells[k] = 0;
    __syncthreads();
  }
  const bool fast_index = aligned16(a.index), fast_ids = aligned16(a.ids);
  PairRun run;                                                            // the lane's run: id, column
  unsigned run_row = 0;                                                   // the id's row
  auto look = [&](bool id_changed, bool) { if (id_changed) run_row = a.rowtab[run.a]; };
  auto flush = [&](unsigned cnt) {
    if (run_row == kDropped) return;
    const int cell = (int)run_row * C + run.b;
    if (dense) atomicAdd(&cells[cell], cnt);
    else atomicAdd(&a.pairs[cell], (int)cnt);
  };
  for_pieces(a.HW, a.span, [&](long long p0, int valid) {
    int v[kPiece], c[kPiece];
    load_ids(a.ids, p0, valid, fast_ids, v);
    load_bytes<false>(a.index + p0, valid, fast_index, c);
#pragma unroll
    for (int k = 0; k < kPiece; ++k) c[k] = min(c[k], a.n);
    walk_pairs(run, v, c, valid, look, flush);
  });
  if (run.cnt) flush(run.cnt);
  if (dense) {
    __syncthreads();
    for (int k = threadIdx.x; k < used; k += kThreads) {
      const unsigned cnt = cells[k];
      if (cnt) atomicAdd(&a.pairs[k], (int)cnt);
    }
  }
}

__global__ __launch_bounds__(CP_WAVE) void pan_area_kernel(const int* __restrict__ pairs, int n, int* __restrict__ seg) {
  const int r = blockIdx.x, C = n + 1;
  if (r > min(seg[0], kMaxRows)) return;
  int sum = 0;
  for (int c = threadIdx.x; c < C; c += CP_WAVE) sum += pairs[r * C + c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, CP_WAVE);
  if (threadIdx.x == 0) seg[r == 0 ? 1 : 4 * r + 3] = sum;
}

__global__ __launch_bounds__(kOneThreads) void pan_match_kernel(MatchTables h, const int* __restrict__ seg,
                                                                const int* __restrict__ pairs, int n, int L,
                                                                long long* __restrict__ stat, double* __restrict__ iou,
                                                                int* __restrict__ bad, int* __restrict__ match) {
  __shared__ double s_iou[kMaxRows + 1];                                  // IoU of a matched row
  __shared__ int s_area[256], s_label[256], s_col_row[256], s_exists[256];
  __shared__ short s_row_col[kMaxRows + 1];                               // matched slot of a row, -1 for none
  __shared__ uint8_t s_row_label[kMaxRows + 1];                           // label | crowd << 7
  __shared__ int s_area_g[kMaxRows + 1], s_cand_inter[kMaxRows + 1];        // a row's area, its candidate's pixels
  __shared__ short s_cand_col[kMaxRows + 1];                              // the only slot that can match the row
  __shared__ int s_crowd_row[kMaxLabels], s_tp[kMaxLabels], s_fp[kMaxLabels], s_fn[kMaxLabels], s_bad;
  __shared__ uint8_t s_flags[kMaxLabels];
  const int t = threadIdx.x;
  const int G = seg[0], C = n + 1;
  if (G > kMaxRows) {                                                     // too many segments: nothing is scored
    if (t == 0) bad[0] += 1;
    if (match && t < n) match[t] = -1;
    return;
  }
  if (t < 256) {
    s_area[t] = 0; s_col_row[t] = 0; s_exists[t] = 0;
    s_label[t] = t < n ? h.pred_label[t] : -1;
  }
  if (t < kMaxLabels) { s_crowd_row[t] = 0; s_tp[t] = 0; s_fp[t] = 0; s_fn[t] = 0; s_flags[t] = t < L ? h.flags[t] : 0; }
  if (t == 0) s_bad = 0;
  for (int r = t; r <= G; r += kOneThreads) {
    s_row_col[r] = -1;
    s_cand_col[r] = -1;
    s_row_label[r] = r ? (uint8_t)(seg[4 * r + 1] | (seg[4 * r + 2] ? 0x80 : 0)) : 0;
    s_area_g[r] = seg[4 * r + 3];
  }
  __syncthreads();
  // ONE pass over the table, cell after cell (coalesced, eight loads in flight per lane): the column areas, and per
  // row the only cell that can match -- 2 inter > union needs 2 inter > area_g, which one cell of a row at most has
  const int cells = (G + 1) * C;
  for (int base = 0; base < cells; base += 8 * kOneThreads) {
    int cnt[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = base + u * kOneThreads + t;
      cnt[u] = f < cells ? pairs[f] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (cnt[u] == 0) continue;
      const int f = base + u * kOneThreads + t, r = f / C, c = f - r * C;
      if (c == n) continue;
      atomicAdd(&s_area[c], cnt[u]);
      if (r >= 1 && 2 * (long long)cnt[u] > (long long)s_area_g[r]) { s_cand_col[r] = (short)c; s_cand_inter[r] = cnt[u]; }
    }
  }
  for (int r = 1 + t; r <= G; r += kOneThreads)                           // the crowd row of a label: the highest value
    if (s_row_label[r] & 0x80) atomicMax(&s_crowd_row[s_row_label[r] & 0x7f], r);
  __syncthreads();
  if (t < n) {
    const int lab = s_label[t];
    const bool ok = lab >= 0 && (s_flags[lab] & 1);
    if (s_area[t] > 0 && !ok) atomicAdd(&s_bad, 1);
    s_exists[t] = s_area[t] > 0 && ok;
  }
  __syncthreads();
  for (int r = 1 + t; r <= G; r += kOneThreads) {
    if (s_row_label[r] & 0x80) continue;                                  // a crowd row: neither matched nor missed
    const int lab = s_row_label[r], c = s_cand_col[r];
    bool matched = false;
    if (c >= 0 && s_exists[c] && s_label[c] == lab) {
      const long long inter = s_cand_inter[r];
      const long long uni = (long long)s_area_g[r] + s_area[c] - inter - pairs[c];
      // integer comparison: for counts below 2^32 it decides exactly as the evaluator's float64 inter / union > 0.5,
      // since the smallest quotient above one half exceeds it by 1 / (2 union) >= 2^-33, far above an ulp of 0.5
      if (2 * inter > uni) {                                              // at most one per row and per column
        s_row_col[r] = (short)c;
        s_col_row[c] = r;
        s_iou[r] = (double)inter / (double)uni;
        matched = true;
      }
    }
    atomicAdd(matched ? &s_tp[lab] : &s_fn[lab], 1);
  }
  __syncthreads();
  if (t < CP_WAVE) {                                                      // the first wave: one lane per label
    // the matched IoUs onto the running sum in ascending row order: 64 rows per ballot, then its set bits in order
    double sum = t < L ? iou[t] : 0.0;
    bool any = false;
    for (int r0 = 1; r0 <= G; r0 += CP_WAVE) {
      const int r = r0 + t;
      unsigned long long mask = __ballot(r <= G && s_row_col[r] >= 0);
      while (mask) {
        const int rr = r0 + __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (s_row_label[rr] == t) { sum += s_iou[rr]; any = true; }
      }
    }
    if (any) iou[t] = sum;
    if (t < L && s_tp[t]) stat[3 * t] += s_tp[t];
    if (t < L && s_fn[t]) stat[3 * t + 2] += s_fn[t];
  }
  if (t < n) {
    if (s_exists[t] && s_col_row[t] == 0) {
      const int lab = s_label[t], rc = s_crowd_row[lab];
      const long long x = (long long)pairs[t] + (rc ? pairs[rc * C + t] : 0);
      if (!(2 * x > (long long)s_area[t])) atomicAdd(&s_fp[lab], 1);      // else more than half VOID and crowd: ignored
    }
    if (match) match[t] = s_exists[t] ? s_col_row[t] : -1;
  }
  __syncthreads();
  if (t < L && s_fp[t]) stat[3 * t + 1] += s_fp[t];
  if (t == 0 && s_bad) bad[1] += s_bad;
}

}  // namespace

extern "C" size_t cp_panoptic_pairs_workspace_bytes(void) {
  return (size_t)kIds + (size_t)kIds * sizeof(uint16_t);                  // the presence bytes, the id -> row table
}

extern "C" int cp_panoptic_pairs(const uint8_t* index, int32_t n, const uint16_t* gt_ids, int32_t H, int32_t W,
                                 int32_t id_divisor, int32_t id_direct_below, int32_t L, const uint8_t* label_flags,
                                 int32_t* seg, int32_t* pairs, void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && L >= 1 && n >= 0 && id_divisor >= 1 && id_direct_below >= 0);
  const long long HW = (long long)H * W;
  if (L > kMaxLabels || n > kMaxSlots || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(index && gt_ids && label_flags && seg && pairs);
  CP_CHECK_ARG(((uintptr_t)gt_ids & 1) == 0 && ((uintptr_t)seg & 15) == 0 && ((uintptr_t)pairs & 3) == 0);
  if (!workspace || workspace_bytes < cp_panoptic_pairs_workspace_bytes()) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  LabelFlags fl;
  for (int k = 0; k < kMaxLabels; ++k) fl.f[k] = k < L ? label_flags[k] : 0;
  uint8_t* presence = (uint8_t*)workspace;
  uint16_t* rowtab = (uint16_t*)(presence + kIds);
  const int cells = (kMaxRows + 1) * (n + 1);
  hipLaunchKernelGGL(pan_clear_kernel, dim3(min((cells + kThreads - 1) / kThreads, 4 * kWorkgroups)), dim3(kThreads), 0,
                     st, (unsigned*)presence, pairs, cells);
  const long long span = span_for(HW, kWorkgroups);
  const unsigned blocks = span_blocks(HW, span);
  hipLaunchKernelGGL(pan_presence_kernel, dim3(blocks), dim3(kThreads), 0, st, gt_ids, HW, span, presence);
  hipLaunchKernelGGL(pan_compact_kernel, dim3(1), dim3(kOneThreads), 0, st, fl, presence, id_divisor, id_direct_below, L,
                     rowtab, seg);
  CountArgs a;
  a.index = index; a.ids = gt_ids; a.rowtab = rowtab; a.seg = seg; a.pairs = pairs; a.HW = HW; a.span = span; a.n = n;
  hipLaunchKernelGGL(pan_count_kernel, dim3(blocks), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(pan_area_kernel, dim3(kMaxRows + 1), dim3(CP_WAVE), 0, st, pairs, n, seg);
  return cp_launch_status();
}

extern "C" int cp_panoptic_match(const int32_t* seg, const int32_t* pairs, int32_t n, const int32_t* pred_label, int32_t L,
                                 const uint8_t* label_flags, int64_t* stat, double* iou, int32_t* bad, int32_t* match,
                                 void* stream) {
  CP_CHECK_ARG(L >= 1 && n >= 0);
  if (L > kMaxLabels || n > kMaxSlots) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(seg && pairs && label_flags && stat && iou && bad && (n == 0 || pred_label));
  CP_CHECK_ARG(((uintptr_t)seg & 3) == 0 && ((uintptr_t)pairs & 3) == 0 && ((uintptr_t)stat & 7) == 0 &&
               ((uintptr_t)iou & 7) == 0 && ((uintptr_t)bad & 3) == 0 && ((uintptr_t)match & 3) == 0);
  MatchTables h;
  for (int k = 0; k < 256; ++k) h.pred_label[k] = k < n && pred_label[k] >= 0 && pred_label[k] < L ? (int16_t)pred_label[k] : -1;
  for (int k = 0; k < kMaxLabels; ++k) h.flags[k] = k < L ? label_flags[k] : 0;
  hipLaunchKernelGGL(pan_match_kernel, dim3(1), dim3(kOneThreads), 0, (hipStream_t)stream, h, seg, pairs, n, L,
                     (long long*)stat, iou, bad, match);
  return cp_launch_status();
}
