// The three full-resolution layers of the DLA base as ONE kernel at inference (gfx950, split-bf16 x3 on the bf16 matrix
// cores): image in, 32 channels at half resolution out.
//
//   s  = relu(conv7x7(image, ws) + bs)        3 -> 16, stride 1, pad 3          (pose_dla_dcn.py:236-246,266-276:
//   y0 = relu(conv3x3(s, w0) + b0)            16 -> 16, stride 1, pad 1          `base_layer`, `base.level0`, `base.level1`,
//   y1 = relu(conv3x3_s2(y0, w1) + b1)        16 -> 32, stride 2, pad 1           BN folded)
//
// Why: as conv_stem_kernel<1,1> + conv_base_pair_kernel the 16-channel stem map (134 MB at 1024 x 2048, one consumer) is
// written and read back between two launches.  Here it stays in LDS like y0 does in the pair kernel, and every element
// goes through the operation sequence of those two kernels: the result is bit-identical to theirs.
//
// One workgroup = 8 waves walks DOWN a column strip of 32 y1 columns, one step = 2 rows of y1.  Rows that two steps share
// stay in LDS rings, so a step computes only what is new (the pair kernel's independent 2-row tiles would recompute 1.8x
// of the 7x7 work):
//   * records: ring of 12 image rows x 3 channels x 72 cells, rec[ci][row][cell] = the 8 image columns cell - 4 .. cell + 3
//     split to bf16 hi | lo (conv_stem.hip's B layout: one ds_read_b128 per fragment half); a step stages 4 new rows from
//     three float4 loads per thread that were issued a step ahead.
//   * stage A (stem): 4 new rows x 67 cells = 16 tiles + one tile for the last 3 cells of the four rows; 6 k-steps of
//     (ky, ci) pairs x 8 columns, hi*hi + hi*lo + lo*hi with the weight operand first; + bs, ReLU, ZERO outside the image
//     (level0's padding), split by psplit2 into the s ring (8 rows x 72 cells, the pair kernel's x region layout).
//   * stage B (level0): 4 new rows x 65 columns = 16 tiles + one tile for column 64; as the pair kernel's, into the y0
//     ring (8 rows x 65 cells).
//   * stage C (level1): wave = (row, 16-column tile, channel half); as the pair kernel's.
//   Ring rows are addressed by the row number relative to the run's origin, so nothing is copied between steps.
//   * a vertical run starts with three warm-up steps (records only; records only; records + stem + level0) that fill
//     the rings through the same code; the host picks the run length so that one run per workgroup covers the map at
//     256 workgroups, with at most ceil(Ho / 32) runs per strip (1024 x 2048: 32 strips x 8 runs of 64 y1 rows, 3 % halo
//     work).
//   * all three weight sets stay in registers as A fragments for the whole launch (48 + 40 + 40 VGPRs: a wave holds
//     one channel half of level1's).
//   * a step is two phases and two barriers: stage A with stage C of the step before; stage B with the records of the
//     step after (image rows loaded a step earlier).
// LDS 88.7 (records) + 36.9 (s) + 33.3 (y0) = 158.8 KB: one workgroup of 8 waves per CU; 254 VGPRs, no scratch.
// 1 x 3 x 1024 x 2048: 132 us in the network against 72.8 + 101.4 us for the two launches.
#include <type_traits>

#include "cp_common.h"

namespace {

typedef __bf16 tbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 tbf16x2 __attribute__((ext_vector_type(2)));
typedef float tf32x2 __attribute__((ext_vector_type(2)));
typedef unsigned tu32x4 __attribute__((ext_vector_type(4)));
typedef unsigned tu32x2 __attribute__((ext_vector_type(2)));

constexpr unsigned TOOB = 0x80000000u;
constexpr int NT = 512, NWG = 256;
constexpr int CIN = 16, C1 = 32, KS = 5;               // the 3x3 layers: 5 k-steps of two taps x 16 channels
constexpr int SKS = 6, SPAIRS = 21;                    // the stem: 6 k-steps of four (ky, ci) pairs x 8 columns
constexpr int TW2 = 32;                                // y1 columns of a strip
constexpr int L0W = 2 * TW2 + 1, LR = 8;               // y0 ring: 8 rows x 65 cells
constexpr int XW = 72, XR = 8;                         // s ring: 8 rows x 72 cells (from the 16-byte aligned column 2 x0 - 4)
constexpr int RR = 12, RP = XW + 5;                    // record ring: 12 rows x 77 slots (a pad slot before cells 2, 18, 34, 50, 66)
constexpr int NSEG = XW / 4;                           // staging segments of 4 records per (channel, row)
constexpr int XHALF = XR * XW * 16, L0HALF = LR * L0W * 16, RPLANE = 3 * RR * RP * 16;
constexpr int LDS_BYTES = 2 * RPLANE + 4 * XHALF + 4 * L0HALF;
static_assert(3 * 4 * NSEG <= NT, "one staging item per thread");
static_assert(C1 * CIN * 9 * 4 <= 2 * RPLANE, "the raw weights fit the region they pass through");
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU");

struct TrioArgs {
  const float* image;   // [B][3][H][W]
  const tbf16x8* wp;    // cp_conv7x7_c3_prepare's fragments, Cout = 16
  const float* bs;      // [16] or null
  const float* w0;      // [16][16][3][3]
  const float* b0;      // [16] or null
  const float* w1;      // [32][16][3][3]
  const float* b1;      // [32] or null
  float* out;           // [B][32][Ho][Wo]
  int H, W, Ho, Wo;
  int strips, run_rows, items_per_image, nitems;
};

// the split of conv_base_pair.hip's x staging (the value alone decides the two halves)
__device__ __forceinline__ void tsplit2(float v0, float v1, unsigned& hi, unsigned& lo) {
  const tbf16x2 h = __builtin_convertvector(tf32x2{v0, v1}, tbf16x2);
  const unsigned hb = __builtin_bit_cast(unsigned, h);
  const float h0 = __builtin_bit_cast(float, hb << 16), h1 = __builtin_bit_cast(float, hb & 0xffff0000u);
  const tbf16x2 l = __builtin_convertvector(tf32x2{v0 - h0, v1 - h1}, tbf16x2);
  hi = hb;
  lo = __builtin_bit_cast(unsigned, l);
}

__device__ __forceinline__ int rslot(int cell) { return cell + ((cell + 14) >> 4); }

__global__ __launch_bounds__(NT, 1) void conv_base_trio_kernel(TrioArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char rec[2 * RPLANE];     // image records [hi | lo][ci][ring row][slot]
  __shared__ __attribute__((aligned(16))) unsigned char xs[4 * XHALF];       // s ring [hi | lo][channel half][ring row][cell]
  __shared__ __attribute__((aligned(16))) unsigned char ls[4 * L0HALF];      // y0 ring

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lpx = lane & 15, g = lane >> 4;
  const int HW = a.H * a.W;
  const int cm = wid & 1;                                            // the wave's channel half of level1

  // ---- once per workgroup: the weights as A fragments in registers
  tbf16x8 sa[SKS][2], wh0[KS], wl0[KS], wh1[KS], wl1[KS];
#pragma unroll
  for (int s_ = 0; s_ < SKS; ++s_) {
    sa[s_][0] = a.wp[(s_ * 2 + 0) * 64 + lane];
    sa[s_][1] = a.wp[(s_ * 2 + 1) * 64 + lane];
  }
  {
    float* wsh = reinterpret_cast<float*>(rec);
    for (int i = tid; i < CIN * CIN * 9; i += NT) wsh[i] = a.w0[i];
    __syncthreads();
    // A[co = lpx][k = 32 s + 8 g + j] = W[co][ci = 8 (g & 1) + j][tap = 2 s + (g >> 1)] (tap 9: zero)
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) {
      const int tap = 2 * s_ + (g >> 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float w = tap < 9 ? wsh[(lpx * CIN + 8 * (g & 1) + j) * 9 + tap] : 0.f;
        const __bf16 h = (__bf16)w;
        wh0[s_][j] = h;
        wl0[s_][j] = (__bf16)(w - (float)h);
      }
    }
    __syncthreads();
    for (int i = tid; i < C1 * CIN * 9; i += NT) wsh[i] = a.w1[i];
    __syncthreads();
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) {
      const int tap = 2 * s_ + (g >> 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float w = tap < 9 ? wsh[((16 * cm + lpx) * CIN + 8 * (g & 1) + j) * 9 + tap] : 0.f;
        const __bf16 h = (__bf16)w;
        wh1[s_][j] = h;
        wl1[s_][j] = (__bf16)(w - (float)h);
      }
    }
    __syncthreads();                                                 // (the first records overwrite the buffer)
  }
  float bsr[4], b0r[4], b1r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bsr[q] = a.bs ? a.bs[4 * g + q] : 0.f;
    b0r[q] = a.b0 ? a.b0[4 * g + q] : 0.f;
    b1r[q] = a.b1 ? a.b1[16 * cm + 4 * g + q] : 0.f;
  }
  // the lane's (ky, ci) row of stem k-step s, as a byte offset into the record plane and a row number
  int sky[SKS], sci[SKS];
#pragma unroll
  for (int s_ = 0; s_ < SKS; ++s_) {
    const int pair = min(4 * s_ + g, SPAIRS - 1);                    // (pairs past 20 carry zero weights: any record will do)
    sky[s_] = pair / 3;
    sci[s_] = (pair - 3 * sky[s_]) * (RR * RP * 16);
  }
  // the lane's tap of 3x3 k-step s: row and column offset
  int tky[KS], tkx[KS];
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) {
    const int tap = min(2 * s_ + (g >> 1), 8);                       // (the padding tap multiplies zero weights)
    tky[s_] = tap / 3;
    tkx[s_] = tap - 3 * tky[s_];
  }

  // the thread's staging item: (channel, row of the step's four, segment of 4 records) of the record ring; on waves
  // 4 .. 7 (wave 0 carries the extra tile of stage B, in whose phase the records are written)
  const int itid = tid - NT / 2;
  const bool item = itid >= 0 && itid < 3 * 4 * NSEG;
  const int ici = max(itid, 0) / (4 * NSEG), irow = (max(itid, 0) / NSEG) & 3, iseg = max(itid, 0) % NSEG;
  f32x4 v[3];

  // a step = (work item, k); a work item = (image, vertical run, strip), strips fastest: the workgroups in flight share
  // their halo columns in L2.  Steps k = -3, -2, -1 are a run's warm-up.
  struct Step {
    int it, k, b, x0, Y0, ns;
  };
  auto decode = [&](Step& s) {
    s.b = s.it / a.items_per_image;
    const int r = s.it - s.b * a.items_per_image;
    const int run = r / a.strips;
    s.x0 = (r - run * a.strips) * TW2;
    s.Y0 = run * a.run_rows;
    s.ns = (min(a.run_rows, a.Ho - s.Y0) + 1) >> 1;
  };
  auto next_step = [&](const Step& s) {
    Step n = s;
    if (s.it >= a.nitems) return n;
    n.k = s.k + 1;
    if (n.k >= s.ns) {
      n.it = s.it + gridDim.x;
      n.k = -3;
      if (n.it < a.nitems) decode(n);
    }
    return n;
  };
  // rows are numbered relative to 2 Y0; the rings are addressed by (row + 24) % 12 and (row + 16) % 8
  auto km12 = [](int k) { return (4 * k + 24) % 12; };
  auto km8 = [](int k) { return (4 * k + 16) & 7; };

  // image rows 2 Y0 + 4 k + 4 .. + 7 (step k's new rows), columns 2 x0 - 8 + 4 seg .. + 11, into the thread's registers
  auto load_item = [&](const Step& s) {
    const int gy = 2 * s.Y0 + 4 * s.k + 4 + irow, gx0 = 2 * s.x0 - 8 + 4 * iseg;
    const bool rok = item && s.it < a.nitems && gy >= 0 && gy < a.H;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.image + (long long)(s.it < a.nitems ? s.b : 0) * 3 * HW), 0, (int)(3u * (unsigned)HW * 4u),
        0x00020000);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int gx = gx0 + 4 * j;                                    // (W % 4 == 0: whole chunks in or out)
      const unsigned off = (rok && gx >= 0 && gx < a.W) ? ((unsigned)ici * (unsigned)HW + (unsigned)(gy * a.W + gx)) * 4u : TOOB;
      v[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
    }
  };
  // ---- the records of step s' four new image rows (relative rows 4 k + 4 ..) from the thread's registers
  auto write_records = [&](const Step& s) {
    if (!item) return;
    unsigned ph[6], pl[6];                                           // packed (column 2 i, 2 i + 1) pairs, hi and lo halves
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      tsplit2(v[j][0], v[j][1], ph[2 * j], pl[2 * j]);
      tsplit2(v[j][2], v[j][3], ph[2 * j + 1], pl[2 * j + 1]);
    }
    int rr = km12(s.k) + 4 + irow;
    rr = rr >= RR ? rr - RR : rr;
    unsigned char* rowp = rec + ((ici * RR + rr) * RP) * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                    // record r starts at column offset r of the twelve
      tu32x4 rh, rl;
      if ((r & 1) == 0) {
        const int p = r / 2;
        rh = tu32x4{ph[p], ph[p + 1], ph[p + 2], ph[p + 3]};
        rl = tu32x4{pl[p], pl[p + 1], pl[p + 2], pl[p + 3]};
      } else {
        const int p = (r - 1) / 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          rh[j] = __builtin_amdgcn_alignbit(ph[p + j + 1], ph[p + j], 16);
          rl[j] = __builtin_amdgcn_alignbit(pl[p + j + 1], pl[p + j], 16);
        }
      }
      unsigned char* dst = rowp + rslot(4 * iseg + r) * 16;
      *reinterpret_cast<tu32x4*>(dst) = rh;
      *reinterpret_cast<tu32x4*>(dst + RPLANE) = rl;
    }
  };

  // ---- stage A: s = relu(conv7x7(image) + bs) on relative rows 4 k + 1 .. 4 k + 4, cells 2 .. 68, into the s ring.
  // A wave takes two tiles (rows w >> 2 and (w >> 2) + 2, cells 2 + 16 (w & 3) ..): two independent MFMA chains;
  // wave 7 adds the tile of cells 66 .. 68 of the four rows (lane = 3 row + cell)
  auto stage_a = [&](const Step& s, auto nc) {
    constexpr int NCH = decltype(nc)::value;
    const int k12 = km12(s.k), k8 = km8(s.k);
    int crow[NCH], ccell[NCH];
    bool cval[NCH];
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      if (n < 2) {
        crow[n] = (wid >> 2) + 2 * n;
        ccell[n] = 2 + 16 * (wid & 3) + lpx;
        cval[n] = true;
      } else {
        const int r = lpx / 3;
        crow[n] = min(r, 3);
        cval[n] = lpx < 12;
        ccell[n] = cval[n] ? 66 + (lpx - 3 * r) : 66;
      }
    }
    f32x4 acc[NCH];
#pragma unroll
    for (int n = 0; n < NCH; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s_ = 0; s_ < SKS; ++s_) {
      tbf16x8 bh[NCH], bl[NCH];
#pragma unroll
      for (int n = 0; n < NCH; ++n) {
        int t = k12 + 10 + crow[n] + sky[s_];                        // image row (4 k + 1 + row) - 3 + ky, + 24
        t = t >= 2 * RR ? t - 2 * RR : (t >= RR ? t - RR : t);
        const unsigned char* p = rec + sci[s_] + (t * RP + rslot(ccell[n])) * 16;
        bh[n] = *reinterpret_cast<const tbf16x8*>(p);
        bl[n] = *reinterpret_cast<const tbf16x8*>(p + RPLANE);
      }
#pragma unroll
      for (int n = 0; n < NCH; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa[s_][0], bh[n], acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NCH; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa[s_][0], bl[n], acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NCH; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa[s_][1], bh[n], acc[n], 0, 0, 0);
    }
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      if (!cval[n]) continue;
      const int sy = 2 * s.Y0 + 4 * s.k + 1 + crow[n], sx = 2 * s.x0 - 4 + ccell[n];
      const bool inside = sy >= 0 && sy < a.H && sx >= 0 && sx < a.W;
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = inside ? cp_relu(acc[n][q] + bsr[q]) : 0.f;
      unsigned hi[2], lo[2];
      tsplit2(o[0], o[1], hi[0], lo[0]);
      tsplit2(o[2], o[3], hi[1], lo[1]);
      // channels 4 g .. 4 g + 3: half g >> 1, elements 4 (g & 1) .. of the cell
      const int rr = (k8 + 1 + crow[n]) & 7;
      unsigned char* dst = xs + (g >> 1) * XHALF + (rr * XW + ccell[n]) * 16 + (g & 1) * 8;
      *reinterpret_cast<tu32x2*>(dst) = tu32x2{hi[0], hi[1]};
      *reinterpret_cast<tu32x2*>(dst + 2 * XHALF) = tu32x2{lo[0], lo[1]};
    }
  };

  // ---- stage B: y0 = relu(conv3x3(s) + b0) on relative rows 4 k .. 4 k + 3, columns 0 .. 64 (image column
  // 2 x0 - 1 + c; column c, tap kx <-> s cell c + kx + 2), into the y0 ring; wave 0 adds the tile of column 64
  auto stage_b = [&](const Step& s, auto nc) {
    constexpr int NCH = decltype(nc)::value;
    const int k8 = km8(s.k);
    int crow[NCH], ccol[NCH];
    bool cval[NCH];
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      if (n < 2) {
        crow[n] = (wid >> 2) + 2 * n;
        ccol[n] = 16 * (wid & 3) + lpx;
        cval[n] = true;
      } else {
        crow[n] = min(lpx, 3);
        ccol[n] = L0W - 1;
        cval[n] = lpx < 4;
      }
    }
    f32x4 acc[NCH];
#pragma unroll
    for (int n = 0; n < NCH; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) {
      tbf16x8 bh[NCH], bl[NCH];
#pragma unroll
      for (int n = 0; n < NCH; ++n) {
        const int rr = (k8 + 7 + crow[n] + tky[s_]) & 7;             // s row (4 k + row) - 1 + ky
        const unsigned char* p = xs + (g & 1) * XHALF + (rr * XW + ccol[n] + 2 + tkx[s_]) * 16;
        bh[n] = *reinterpret_cast<const tbf16x8*>(p);
        bl[n] = *reinterpret_cast<const tbf16x8*>(p + 2 * XHALF);
      }
#pragma unroll
      for (int n = 0; n < NCH; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh0[s_], bh[n], acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NCH; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh0[s_], bl[n], acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NCH; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl0[s_], bh[n], acc[n], 0, 0, 0);
    }
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      if (!cval[n]) continue;
      const int iy = 2 * s.Y0 + 4 * s.k + crow[n], ix = 2 * s.x0 - 1 + ccol[n];
      const bool inside = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = inside ? cp_relu(acc[n][q] + b0r[q]) : 0.f;
      unsigned hi[2], lo[2];
      tsplit2(o[0], o[1], hi[0], lo[0]);
      tsplit2(o[2], o[3], hi[1], lo[1]);
      const int rr = (k8 + crow[n]) & 7;
      unsigned char* dst = ls + (g >> 1) * L0HALF + (rr * L0W + ccol[n]) * 16 + (g & 1) * 8;
      *reinterpret_cast<tu32x2*>(dst) = tu32x2{hi[0], hi[1]};
      *reinterpret_cast<tu32x2*>(dst + 2 * L0HALF) = tu32x2{lo[0], lo[1]};
    }
  };

  // ---- stage C: y1 = relu(conv_s2(y0) + b1), rows Y0 + 2 k, + 1: wave = (row wid >> 2, 16-column tile, channel half)
  auto stage_c = [&](const Step& s) {
    const int k8 = km8(s.k);
    const int row = wid >> 2, x2 = ((wid >> 1) & 1) * 16 + lpx;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) {
      const int rr = (k8 + 7 + 2 * row + tky[s_]) & 7;               // y0 row (4 k + 2 row) - 1 + ky
      const unsigned char* p = ls + (g & 1) * L0HALF + (rr * L0W + 2 * x2 + tkx[s_]) * 16;
      const tbf16x8 bh = *reinterpret_cast<const tbf16x8*>(p);
      const tbf16x8 bl = *reinterpret_cast<const tbf16x8*>(p + 2 * L0HALF);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh1[s_], bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh1[s_], bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl1[s_], bh, acc, 0, 0, 0);
    }
    const int oy = s.Y0 + 2 * s.k + row, ox = s.x0 + x2;
    if (oy < a.Ho && ox < a.Wo) {
      float* ob = a.out + (long long)s.b * C1 * a.Ho * a.Wo;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        ob[((long long)(16 * cm + 4 * g + q) * a.Ho + oy) * a.Wo + ox] = cp_relu(acc[q] + b1r[q]);
    }
  };

  // ---- the workgroup's steps, two phases and two barriers each:
  //   phase 1: stage A of this step and stage C of the previous one (they share nothing);
  //   phase 2: stage B of this step, the records of the next step (its image rows were loaded a step ago), and the loads
  //            of the step after that.
  // Stage C reads the y0 rows stage B wrote a phase earlier; stage B's next writes come two barriers later.  The records
  // written in phase 2 replace rows that stage A (phase 1) read last; stage A's next writes to the s ring follow stage B's
  // reads by a barrier.
  // The warm-up step k = -1 runs stage B over the y0 rows -4 .. -1 of the run; stage C reads only row -1 of them.  Rows
  // -4 and -3 come from s ring rows the run has not written yet: don't-care values (an MFMA column depends on its own B
  // column alone), overwritten before anything reads them.
  Step prv, cur, nxt;
  cur.it = blockIdx.x;
  cur.k = -3;
  cur.b = cur.x0 = cur.Y0 = cur.ns = 0;
  decode(cur);                                                       // (the grid has no more workgroups than items)
  prv = cur;                                                         // (k < 0: no stage C)
  load_item(cur);
  write_records(cur);
  nxt = next_step(cur);
  load_item(nxt);
  __syncthreads();
#pragma unroll 1
  while (cur.it < a.nitems) {
    if (cur.k >= -1) {
      if (wid == 7) stage_a(cur, std::integral_constant<int, 3>());
      else stage_a(cur, std::integral_constant<int, 2>());
    }
    if (prv.k >= 0) stage_c(prv);
    __syncthreads();                                                 // s rows complete
    if (cur.k >= -1) {
      if (wid == 0) stage_b(cur, std::integral_constant<int, 3>());
      else stage_b(cur, std::integral_constant<int, 2>());
    }
    if (nxt.it < a.nitems) write_records(nxt);
    const Step n2 = next_step(nxt);
    load_item(n2);
    __syncthreads();                                                 // y0 rows complete, the next step's records staged
    prv = cur;
    cur = nxt;
    nxt = n2;
  }
  if (prv.k >= 0) stage_c(prv);
}

}  // namespace

extern "C" int cp_dla_base_trio_supported(int32_t H, int32_t W) {
  return H >= 1 && W >= 4 && (W & 3) == 0 && (unsigned long long)CIN * H * W * 4ull < 0x70000000ull;
}

// out = relu(conv3x3 stride 2 (relu(conv3x3(relu(conv7x7(image) + bs), w0) + b0), w1) + b1):
// image [B][3][H][W] -> out [B][32][(H-1)/2+1][(W-1)/2+1]
extern "C" int cp_dla_base_trio_forward(const float* image, const void* stem_wperm, const float* stem_bias, const float* w0,
                                        const float* b0, const float* w1, const float* b1, float* out, int32_t B, int32_t H,
                                        int32_t W, void* stream) {
  CP_CHECK_ARG(image && stem_wperm && w0 && w1 && out && B >= 1 && B <= 65535);
  if (!cp_dla_base_trio_supported(H, W) || (reinterpret_cast<unsigned long long>(image) & 15)) return CP_EUNSUPPORTED;
  TrioArgs a;
  a.image = image; a.wp = (const tbf16x8*)stem_wperm; a.bs = stem_bias;
  a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1; a.out = out;
  a.H = H; a.W = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
  a.strips = (a.Wo + TW2 - 1) / TW2;
  // vertical runs: as many per strip as it takes to give every workgroup one (a run's warm-up recomputes one step of the
  // stem and of level0), but at most ceil(Ho / 32) runs per strip, each of an even number of y1 rows (Ho = 100: 4 runs
  // of 26).  The 256 workgroups share the items evenly only where strips x runs x B divides into them: B = 3 at
  // 1024 x 2048 is 288 items, two rounds.
  const long long columns = (long long)a.strips * B;
  long long nruns = (NWG + columns - 1) / columns;
  const long long cap = (a.Ho + 31) / 32;
  nruns = nruns < cap ? nruns : cap;
  int rows = (int)((a.Ho + nruns - 1) / nruns);
  rows += rows & 1;
  a.run_rows = rows;
  a.items_per_image = a.strips * ((a.Ho + rows - 1) / rows);
  const long long nitems = (long long)a.items_per_image * B;
  if (nitems > 0x3FFFFFFFll) return CP_EUNSUPPORTED;
  a.nitems = (int)nitems;
  const int wgs = (int)(nitems < NWG ? nitems : NWG);               // one workgroup per CU, each a run of items
  hipLaunchKernelGGL(conv_base_trio_kernel, dim3(wgs), dim3(NT), 0, (hipStream_t)stream, a);
  return cp_launch_status();
}
