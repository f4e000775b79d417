// Pixel counting of the pixel-level evaluation (evalPixelLevelSemanticLabeling of the cityscapesscripts and the
// kittiscripts) for gfx950: the confusion matrix of one image, added to a matrix that stays on the device, and the
// (size, tp, category tp) row of every ground-truth instance of interest, from the 8-bit prediction and the 16-bit
// instance-id image in one pass over both.
//   pixel_prepare_kernel    64 workgroups build the 65536-entry table id -> (instance column, ground-truth label, that
//                           label's group) in the workspace: a workgroup writes its 1024 entries, then enters the ids
//                           of `inst_ids` that fall into its own range, so no workgroup waits for another.  The first
//                           one also turns pred_label / label_group into the 256-entry table prediction byte ->
//                           (label, group) and zeroes `inst`.
//   pixel_confusion_kernel  one workgroup per CU over a span of pixels.  A lane takes 16 consecutive pixels per step
//                           and keeps ONE run (id, prediction byte, count) in registers across all its steps; it
//                           touches the counters in LDS (L x L for the matrix, 3 x G for the instances) only when the
//                           id or the prediction changes: a street scene's pixels land in a handful of bins, and a
//                           per-pixel add would serialise on them.  A value is looked up only when it differs from the
//                           one before.  At the end the workgroup sends its non-zero counters to global memory, one
//                           atomic per bin and workgroup.
// Two launches, whatever G.  Integer atomics only: the result does not depend on the order of the additions.
// The piece, span and run scheme, the loaders and the run walker are pixel_pieces.h's.
#include "pixel_pieces.h"

namespace {

constexpr int kPrepBlocks = 64, kPrepThreads = 1024;    // kPrepBlocks * kPrepThreads == kIds
constexpr int kMaxLabels = 64, kMaxInst = 1024;
constexpr unsigned kNone = 0xff;                        // label / group code: outside the table / no group
constexpr unsigned kNoColumn = 0xffff;
constexpr int kWorkgroups = 256;                        // one per CU: every workgroup ends with atomics on the same few bins

// table entry of an id: column | label << 16 | group << 24;  of a prediction byte: label | group << 8
struct HostTables {
  uint8_t pred_label[256];
  int8_t label_group[kMaxLabels];
};

__global__ __launch_bounds__(kPrepThreads) void pixel_prepare_kernel(HostTables t, const int* __restrict__ inst_ids,
                                                                     int G, int id_divisor, int id_direct_below, int L,
                                                                     unsigned* __restrict__ table,
                                                                     unsigned* __restrict__ ptab,
                                                                     int* __restrict__ inst) {
  __shared__ unsigned group[kMaxLabels];                                  // label -> group code
  const int x = threadIdx.x;
  if (x < kMaxLabels) group[x] = x < L && t.label_group[x] >= 0 ? (unsigned)t.label_group[x] : kNone;
  __syncthreads();
  const int v = blockIdx.x * kPrepThreads + x;                            // < kIds
  const int g = v < id_direct_below ? v : v / id_divisor;
  const unsigned gc = g < L ? (unsigned)g : kNone;
  table[v] = kNoColumn | gc << 16 | (gc == kNone ? kNone : group[gc]) << 24;
  if (blockIdx.x == 0) {
    if (x < 256) {
      const unsigned p = t.pred_label[x] < L ? (unsigned)t.pred_label[x] : kNone;
      ptab[x] = p | (p == kNone ? kNone : group[p]) << 8;
    }
    for (int k = x; k < 3 * G; k += kPrepThreads) inst[k] = 0;
  }
  __syncthreads();                                                        // this workgroup's entries are written
  if (x < G) {
    const int id = inst_ids[x];                                           // distinct: one writer per entry
    const int first = (int)blockIdx.x * kPrepThreads;                     // (an id outside 16 bits matches no pixel)
    if (id >= first && id < first + kPrepThreads)
      table[id] = (table[id] & 0xffff0000u) | (unsigned)x;
  }
}

struct PixelArgs {
  const uint8_t* pred;        // [HW]
  const uint16_t* ids;        // [HW]
  const unsigned* table;      // [65536]
  const unsigned* ptab;       // [256]
  unsigned long long* conf;   // [L][L]
  int* inst;                  // [G][3]
  int* bad;                   // [2]
  long long HW, span;         // pixels, pixels per workgroup (a multiple of kTile)
  int L, G;
};

// one run of `cnt` pixels of id entry `e` under prediction entry `pe` into the workgroup's counters
__device__ __forceinline__ void count_run(unsigned e, unsigned pe, unsigned cnt, int L, unsigned* s_conf,
                                          unsigned* s_inst, unsigned& bad0, unsigned& bad1) {
  const unsigned g = e >> 16 & 0xff, gg = e >> 24, col = e & 0xffff, p = pe & 0xff, pg = pe >> 8 & 0xff;
  if (g == kNone) bad0 += cnt;
  else if (p == kNone) bad1 += cnt;
  else atomicAdd(&s_conf[g * L + p], cnt);
  if (col != kNoColumn) {
    atomicAdd(&s_inst[3 * col], cnt);
    if (p != kNone && g != kNone) {
      if (p == g) atomicAdd(&s_inst[3 * col + 1], cnt);
      if (gg != kNone && gg == pg) atomicAdd(&s_inst[3 * col + 2], cnt);
    }
  }
}

__global__ __launch_bounds__(kThreads) void pixel_confusion_kernel(PixelArgs a) {
  extern __shared__ unsigned counters[];                                  // [L * L] matrix, [3 * G] instances
  __shared__ unsigned s_ptab[256], s_bad[2];
  const int nconf = a.L * a.L, nall = nconf + 3 * a.G;
  for (int k = threadIdx.x; k < nall; k += kThreads) counters[k] = 0;
  s_ptab[threadIdx.x] = a.ptab[threadIdx.x];
  if (threadIdx.x < 2) s_bad[threadIdx.x] = 0;
  __syncthreads();
  unsigned* s_conf = counters;
  unsigned* s_inst = counters + nconf;
  const bool fast_pred = aligned16(a.pred), fast_ids = aligned16(a.ids);
  PairRun run;                                                            // the lane's run: id, prediction byte
  unsigned run_e = 0, run_pe = 0, bad0 = 0, bad1 = 0;                     // their entries
  auto look = [&](bool id_changed, bool pred_changed) {
    if (id_changed) run_e = a.table[run.a];
    if (pred_changed) run_pe = s_ptab[run.b];
  };
  auto flush = [&](unsigned cnt) { count_run(run_e, run_pe, cnt, a.L, s_conf, s_inst, bad0, bad1); };
  for_pieces(a.HW, a.span, [&](long long p0, int valid) {
    int v[kPiece], q[kPiece];
    load_ids(a.ids, p0, valid, fast_ids, v);
    load_bytes<false>(a.pred + p0, valid, fast_pred, q);
    walk_pairs(run, v, q, valid, look, flush);
  });
  if (run.cnt) flush(run.cnt);
  if (bad0) atomicAdd(&s_bad[0], bad0);
  if (bad1) atomicAdd(&s_bad[1], bad1);
  __syncthreads();
  for (int k = threadIdx.x; k < nall; k += kThreads) {
    const unsigned c = counters[k];
    if (!c) continue;
    if (k < nconf) atomicAdd(&a.conf[k], (unsigned long long)c);
    else atomicAdd(&a.inst[k - nconf], (int)c);
  }
  if (threadIdx.x < 2 && s_bad[threadIdx.x]) atomicAdd(&a.bad[threadIdx.x], (int)s_bad[threadIdx.x]);
}

}  // namespace

extern "C" size_t cp_pixel_confusion_workspace_bytes(int32_t G) {
  (void)G;
  return (size_t)(kIds + 256) * sizeof(unsigned);                         // the id table and the prediction table
}

extern "C" int cp_pixel_confusion(const uint8_t* pred, const uint8_t* pred_label, const uint16_t* gt_ids, int32_t H,
                                  int32_t W, int32_t id_divisor, int32_t id_direct_below, int32_t L,
                                  const int8_t* label_group, const int32_t* inst_ids, int32_t G, int64_t* conf,
                                  int32_t* inst, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && L >= 1 && G >= 0 && id_divisor >= 1 && id_direct_below >= 0);
  const long long HW = (long long)H * W;
  if (L > kMaxLabels || G > kMaxInst || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(pred && pred_label && gt_ids && label_group && conf && bad && (G == 0 || (inst_ids && inst)));
  CP_CHECK_ARG(((uintptr_t)gt_ids & 1) == 0 && ((uintptr_t)conf & 7) == 0);
  if (!workspace || workspace_bytes < cp_pixel_confusion_workspace_bytes(G)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  HostTables t;
  for (int k = 0; k < 256; ++k) t.pred_label[k] = pred_label[k];
  for (int k = 0; k < kMaxLabels; ++k) t.label_group[k] = k < L ? label_group[k] : (int8_t)-1;
  unsigned* table = (unsigned*)workspace;
  unsigned* ptab = table + kIds;
  hipLaunchKernelGGL(pixel_prepare_kernel, dim3(kPrepBlocks), dim3(kPrepThreads), 0, st, t, inst_ids, G, id_divisor,
                     id_direct_below, L, table, ptab, inst);
  PixelArgs a;
  a.pred = pred; a.ids = gt_ids; a.table = table; a.ptab = ptab; a.conf = (unsigned long long*)conf; a.inst = inst;
  a.bad = bad; a.HW = HW; a.L = L; a.G = G;
  a.span = span_for(HW, kWorkgroups);
  hipLaunchKernelGGL(pixel_confusion_kernel, dim3(span_blocks(HW, a.span)), dim3(kThreads),
                     (size_t)(L * L + 3 * G) * sizeof(unsigned), st, a);
  return cp_launch_status();
}
