// 3x3 / stride 1 / pad 1 forward convolution of one float32 NCHW source to <= 32 output channels, streamed through
// registers (gfx950): the 27-channel `conv_offset_mask` of the DCN modules at inference (reference:
// src/lib/models/networks/DCNv2/dcn_v2.py:137-145), + bias, float32 NCHW out.
//
// Why a kernel of its own: with <= 32 output channels these launches are a few hundred workgroup-chunks of almost no
// matrix work, and conv_mfma_kernel<2, RW, 9, KS> walks them as a dependent chain -- per 32-channel chunk a barrier, a
// staging round trip with nothing under it, a barrier, then nine tap steps each behind a weight-fragment load issued one
// tap earlier.  Here nothing is staged and nothing waits for a neighbour -- and every output element is
// the SAME sequence of floating-point operations as in that kernel, so the two give the same bits:
//
//   * The contraction is conv_mfma_kernel's: v_mfma_f32_16x16x32_bf16 with the pixels on the M side and the channels on
//     the N side, 32-channel chunks in ascending order, the taps 0 .. 8 in order inside a chunk, three products per tap in
//     its order (x_hi w_hi, x_lo w_hi, x_hi w_lo), its split of a float into bf16 halves, its prepared weights
//     (cp_conv_mfma_prepare, taps = 9) read as they are, positions outside the image multiplied as zeros (not skipped),
//     its epilogue (+ bias).  Its in-workgroup K split is kept too: KS wave groups take the chunks q, q + KS, ... and the
//     partial tiles are added in group order -- the caller passes the KS that kernel would pick.
//   * A wave owns NT tiles of 16 consecutive pixels of one image row.  Lane (pixel = lane & 15, group = lane >> 4) loads
//     the channels 8 group .. 8 group + 7 of the chunk at its pixel's tap-shifted position -- eight dword buffer loads from
//     eight planes, 4 x 64 contiguous bytes per wave instruction -- and those eight values ARE its A fragment of that tap.
//   * One step = one tap of one chunk.  The loads of the wave's step DEPTH steps ahead are issued around the MFMAs of the
//     current one: the activations before them, the weight fragments right after, into the registers those MFMAs read.
//     Both run at the same depth (conv_stream.hip: the vector memory counter retires in issue order).  The step loop is
//     one basic block: tap and chunk of the step being issued are scalar counters, the halo is a select.
//   * Every global access of a tensor is a buffer access with range checking, the whole byte offset in the vector
//     offset.  A position above / below the image or left / right of its row, a lane past the row's end, a step past the
//     wave's range get the offset OOB = 2^31, a channel past Cin lies past num_records by itself: loads return 0, stores
//     are dropped.  (A column left of 0 or right of W - 1 is a real address of the neighbouring row in the flat plane:
//     that one is forced to OOB per lane and tap.)
//   * A workgroup is four waves: 4 / KS neighbouring wave tiles x KS waves per tile.  The partial tiles of a K split
//     meet in LDS once, after the loop: the only LDS and the only barrier of the kernel.
//   * That is the TAP form (conv3x3_stream_kernel<NT, KS>, NT = 1 | 2 | 4).  Where the width is a multiple of 4, four
//     tiles per wave run as the ROW form instead (conv3x3_stream_row4_kernel<KS>, below): 64 consecutive pixels per wave,
//     16-byte loads, one split per image row and the dx = -1 / +1 operands by DPP row shifts.  Same operations per output
//     element again -- which pixel sits in which row of an MFMA tile changes no bit.
#include <type_traits>

#include "cp_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 32;                    // input channels per chunk (one 16x16x32 MFMA), as in conv_mfma.hip
constexpr int TAPS = 9;
constexpr int MT = 2;                     // 16-channel weight tiles: Cout <= 32
constexpr unsigned OOB = 0x80000000u;     // past every num_records (< 2^31), also with a channel offset (< 2^31) added

// Steps of loads in flight per wave in the tap form.  Two: that form is bound by the rate of its dword loads, not by
// their latency -- depths 1 to 3 measured alike, 4 and 5 slower.
constexpr int DEPTH_TAP = 2;

struct Stream3Args {
  const float* x;              // [B][Cin][H][W]
  const bf16x8* wp;            // cp_conv_mfma_prepare's fragments, taps = 9
  const float* bias;           // [Cout] or null
  float* out;                  // [B][Cout][H][W]
  int Cin, Cout, H, W, nchunk, tpr, ntiles, vec;      // tpr: 16-pixel tiles per image row; ntiles = H tpr
  int tpr4, ntiles4;                                  // the row form's wave tiles of 64 pixels: per image row, in all
};

// fp32 pair -> bf16 hi pair + bf16 lo pair: hi = bf16(v), lo = bf16(v - hi), round to nearest even -- the split of
// conv_mfma_kernel's staging (and conv_stream.hip's split2)
__device__ __forceinline__ void split2(float v0, float v1, unsigned& hi, unsigned& lo) {
  const bf16x2 h = __builtin_convertvector(f32x2{v0, v1}, bf16x2);
  const unsigned hb = __builtin_bit_cast(unsigned, h);
  const float h0 = __builtin_bit_cast(float, hb << 16), h1 = __builtin_bit_cast(float, hb & 0xffff0000u);
  const bf16x2 l = __builtin_convertvector(f32x2{v0 - h0, v1 - h1}, bf16x2);
  hi = hb;
  lo = __builtin_bit_cast(unsigned, l);
}

// Workgroup = 4 waves = 4 / KS neighbouring wave tiles (NT tiles of 16 pixels x 32 output channels each) x KS waves per
// wave tile; wave q of a tile takes the chunks q, q + KS, ...
template <int NT, int KS>
__global__ __launch_bounds__(256, 2) void conv3x3_stream_kernel(Stream3Args a) {
  constexpr int PG = 4 / KS, DEPTH = DEPTH_TAP;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = wave % KS, grp = wave / KS;
  const int c = lane & 15, g = lane >> 4;
  // XCD-aware order (conv_mfma.hip): logical neighbours -- tiles of the same and the next rows -- share an XCD, and with
  // it the halo rows' lines in L2
  int lw = blockIdx.x;
  if ((gridDim.x & 7) == 0) lw = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int T0 = (lw * PG + grp) * NT, b = blockIdx.y;         // first tile of the wave (a tile past the map: all lanes OOB)
  const int W = a.W, H = a.H, HW = H * W;
  const unsigned plane = (unsigned)HW * 4u;

  // tile n: its row (wave-uniform), this lane's pixel in the first channel of its group of eight, the lane's place in the row
  // (edge: bit dx set = the tap column dx is outside the row for this lane -- column 0 has no left neighbour, column
  //  W - 1 no right one, a lane past the row's end has nothing)
  int ty[NT];
  unsigned vin[NT], edge[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int T = T0 + n;
    ty[n] = T < a.ntiles ? T / a.tpr : -4;                    // (-4: every tap's row is outside the image)
    const int x = (T % a.tpr) * 16 + c;
    edge[n] = x >= W ? 7u : (x == 0 ? 1u : 0u) | (x == W - 1 ? 4u : 0u);
    vin[n] = ((unsigned)(8 * g) * (unsigned)HW + (unsigned)(ty[n] * W + x)) * 4u;
  }

  // the fragments of (chunk, tap) of weight tile m: 2 x 64 lanes x 16 bytes at ((m nchunk + chunk) 9 + tap) 2048
  const unsigned tbytes = (unsigned)a.nchunk * TAPS * 2048u, wlane = (unsigned)lane * 16u;
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(a.wp), 0, (int)(MT * tbytes), 0x00020000);
  const int nmine = a.nchunk > q ? (a.nchunk - q + KS - 1) / KS : 0;          // chunks of this wave: q, q + KS, ...
  const int nsteps = nmine * TAPS;
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x + (long long)b * a.Cin * HW), 0, (int)((unsigned)a.Cin * plane), 0x00020000);

  // The loads of the wave's step (its chunk number ic, tap it): 8 NT activation dwords (issue_x) and the 4 weight
  // fragments (issue_w).  Past the wave's range both get the offset OOB: no memory traffic, zeros.  Everything that
  // depends on the step is a scalar select, not a branch.
  int ic = 0, it = 0;                                          // the step the next issue_x / issue_w pair loads
  auto issue_x = [&](float (&v)[NT][8]) __attribute__((always_inline)) {
    const bool live = ic < nmine;
    const int dy = (it * 11) >> 5, dx = it - 3 * dy;          // it / 3, it % 3 for it < 9
    const unsigned delta = (unsigned)(((dy - 1) * W + (dx - 1)) * 4);
    const unsigned cbase = (unsigned)(live ? (q + ic * KS) * KC : 0) * plane;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int yy = ty[n] + dy - 1;
      const bool rowok = live && yy >= 0 && yy < H;             // (wave-uniform)
      const unsigned bad = rowok ? (edge[n] >> dx) & 1u : 1u;
      const unsigned vo = bad ? OOB : vin[n] + delta;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[n][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, vo + (cbase + (unsigned)j * plane), 0, 0));
    }
  };
  auto issue_w = [&](bf16x8 (&w)[MT][2]) __attribute__((always_inline)) {
    const unsigned wo = ic < nmine ? wlane + (unsigned)((q + ic * KS) * TAPS + it) * 2048u : OOB;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      w[m][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wo + (unsigned)m * tbytes, 0, 0));
      w[m][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wo + (unsigned)m * tbytes + 1024u, 0, 0));
    }
    const bool wrap = it == TAPS - 1;                          // on to the next step
    it = wrap ? 0 : it + 1;
    ic += wrap ? 1 : 0;
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  float v[DEPTH][NT][8];
  bf16x8 w[DEPTH][MT][2];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {       // (in the loop's own issue order: its waits are counted from both ways in)
    issue_x(v[d]);
    __builtin_amdgcn_sched_barrier(0);
    issue_w(w[d]);
    __builtin_amdgcn_sched_barrier(0);
  }

  // No guard inside: a step past the range multiplies the zeros its loads returned (at most DEPTH - 1 of them per wave;
  // x + 0 leaves every bit of x).
  for (int s = 0; s < nsteps; s += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      bf16x8 xh[NT], xl[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split2(v[d][n][2 * j], v[d][n][2 * j + 1], hi[j], lo[j]);
        xh[n] = __builtin_bit_cast(bf16x8, hi);
        xl[n] = __builtin_bit_cast(bf16x8, lo);
      }
      issue_x(v[d]);                                            // DEPTH steps ahead, before this step's MFMAs
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[n], w[d][m][0], acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl[n], w[d][m][0], acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[n], w[d][m][1], acc[m][n], 0, 0, 0);
        }
      // the fragments are reloaded in place once the MFMAs have read them (conv_stream.hip)
      __builtin_amdgcn_sched_barrier(0);
      issue_w(w[d]);
    }
  }

  // ------------------------------------------------------------------ epilogue: D[pixel 4 g + r][co = 16 m + c]
  // Tile t = m NT + n of the wave tile is finished by wave t % KS of its group.
  constexpr int NTILE = MT * NT;
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(a.out + (long long)b * a.Cout * HW, 0,
                                                                        (int)((unsigned)a.Cout * plane), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias ? a.Cout * 4 : 0, 0x00020000);
  // K split: the partial tiles go to LDS, once (added below in group order: conv_mfma_kernel's acc0 += acc1, += acc2 ...)
  __shared__ f32x4 red[KS > 1 ? 4 * NTILE * 64 : 1];           // [wave][tile][lane]
  if constexpr (KS > 1) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) red[(wave * NTILE + m * NT + n) * 64 + lane] = acc[m][n];
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = m * 16 + c;
    const float bv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_b, (unsigned)co * 4u, 0, 0));
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int t = m * NT + n;
      if (KS > 1 && t % KS != q) continue;                      // (wave-uniform)
      f32x4 s = acc[m][n];
      if constexpr (KS > 1) {
        s = red[((grp * KS + 0) * NTILE + t) * 64 + lane];
#pragma unroll
        for (int k = 1; k < KS; ++k) s += red[((grp * KS + k) * NTILE + t) * 64 + lane];
      }
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = s[r] + bv;
      // four consecutive pixels of channel co in the tile's row (a tile past the map, a channel past Cout: nothing)
      const int T = T0 + n, x = (T % a.tpr) * 16 + 4 * g;
      const bool ok = T < a.ntiles && co < a.Cout;
      const unsigned off = ((unsigned)co * (unsigned)HW + (unsigned)(ty[n] * W + x)) * 4u;
      if (a.vec) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_o, ok && x < W ? off : OOB, 0, 0);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)o[r]), rs_o,
                                                ok && x + r < W ? off + 4u * r : OOB, 0, 0);
      }
    }
  }
}

// lanes of a DPP row (16 lanes: the pixels of a tile) moved by one; a lane without a source keeps `old`
__device__ __forceinline__ unsigned row_from_left(unsigned old, unsigned src) {       // lane c <- lane c - 1 (row_shr:1)
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)src, 0x111, 0xF, 0xF, false);
}
__device__ __forceinline__ unsigned row_from_right(unsigned old, unsigned src) {      // lane c <- lane c + 1 (row_shl:1)
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)src, 0x101, 0xF, 0xF, false);
}

// The row form, for maps whose width is a multiple of 4: the wave tile is 64 CONSECUTIVE pixels of one image row, and its
// four 16-pixel MFMA tiles are interleaved -- lane c owns the pixels X0 + 4 c .. + 3, pixel e of them is row c of tile e
// (the rows of an MFMA tile are independent outputs: which pixel sits in which row changes no bit).  One step = one
// image row dy of one chunk = the three taps (dy, 0..2):
//   * eight 16-byte loads bring the lane's four pixels of its eight channels (16 lanes x 16 B contiguous per plane),
//     eight dword loads the halo -- lane 0 the pixel left of the wave tile, lane 15 the pixel right of it (or OOB: zero);
//   * the 40 values are split ONCE; tap dx = 1 multiplies them as they are, dx = 0 takes tile e - 1 for tile e and, for
//     tile 0, tile 3 of the lane to the left (DPP row shift; lane 0 keeps the halo), dx = 2 mirrors that;
//   * 72 MFMAs per step; the loads of the next step are issued around them (one register set, two waves per SIMD).
// A quarter of the vector-memory instructions and a third of the split arithmetic of the tap form per MFMA.
template <int KS>
__global__ __launch_bounds__(256, 2) void conv3x3_stream_row4_kernel(Stream3Args a) {
  constexpr int PG = 4 / KS, NT = 4, NTILE = MT * NT;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = wave % KS, grp = wave / KS;
  const int c = lane & 15, g = lane >> 4;
  int lw = blockIdx.x;
  if ((gridDim.x & 7) == 0) lw = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int T = lw * PG + grp, b = blockIdx.y;                 // the wave tile (past the map: all lanes OOB)
  const int W = a.W, H = a.H, HW = H * W;
  const unsigned plane = (unsigned)HW * 4u;
  const int ty = T < a.ntiles4 ? T / a.tpr4 : -4;              // (-4: every tap's row is outside the image)
  const int X0 = (T % a.tpr4) * 64, x = X0 + 4 * c;
  const int hx = c == 0 ? X0 - 1 : c == 15 ? X0 + 64 : -1;     // this lane's halo pixel
  // byte offsets in the row ty of the first channel of the lane's group of eight, or OOB (W % 4 == 0: the four pixels
  // are all inside the row or all outside).  (OOB +- one row + a channel offset is still past num_records.)
  const unsigned vin = x < W ? ((unsigned)(8 * g) * (unsigned)HW + (unsigned)(ty * W + x)) * 4u : OOB;
  const unsigned hin = hx >= 0 && hx < W ? ((unsigned)(8 * g) * (unsigned)HW + (unsigned)(ty * W + hx)) * 4u : OOB;

  const unsigned tbytes = (unsigned)a.nchunk * TAPS * 2048u, wlane = (unsigned)lane * 16u;
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8*>(a.wp), 0, (int)(MT * tbytes), 0x00020000);
  const int nmine = a.nchunk > q ? (a.nchunk - q + KS - 1) / KS : 0;
  const int nsteps = nmine * 3;
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x + (long long)b * a.Cin * HW), 0, (int)((unsigned)a.Cin * plane), 0x00020000);

  int ic = 0, ir = 0;                                          // the step the next issue_x / issue_w pair loads
  auto issue_x = [&](f32x4 (&cv)[8], float (&hv)[8]) __attribute__((always_inline)) {
    const bool live = ic < nmine;
    const int yy = ty + ir - 1;
    const bool rowok = live && yy >= 0 && yy < H;               // (wave-uniform)
    const unsigned rdelta = (unsigned)((ir - 1) * W * 4);
    const unsigned cbase = (unsigned)(live ? (q + ic * KS) * KC : 0) * plane;
    const unsigned vo = rowok ? vin + rdelta : OOB, ho = rowok ? hin + rdelta : OOB;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cv[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, vo + (cbase + (unsigned)j * plane), 0, 0));
      hv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, ho + (cbase + (unsigned)j * plane), 0, 0));
    }
  };
  // (the fragments of tap dx of the step: each tap's are reloaded as soon as its MFMAs have read them)
  auto issue_w = [&](int t, bf16x8 (&w)[MT][2]) __attribute__((always_inline)) {
    const unsigned wo = ic < nmine ? wlane + (unsigned)((q + ic * KS) * TAPS + 3 * ir + t) * 2048u : OOB;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      w[m][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wo + (unsigned)m * tbytes, 0, 0));
      w[m][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wo + (unsigned)m * tbytes + 1024u, 0, 0));
    }
  };
  auto next_step = [&]() __attribute__((always_inline)) {
    const bool wrap = ir == 2;
    ir = wrap ? 0 : ir + 1;
    ic += wrap ? 1 : 0;
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int e = 0; e < NT; ++e) acc[m][e] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 cv[8];
  float hv[8];
  bf16x8 w[3][MT][2];
  issue_x(cv, hv);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < 3; ++t) issue_w(t, w[t]);
  next_step();
  __builtin_amdgcn_sched_barrier(0);

  for (int s = 0; s < nsteps; ++s) {
    unsigned ch[NT][4], cl[NT][4], hh[4], hl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int e = 0; e < NT; ++e) split2(cv[2 * k][e], cv[2 * k + 1][e], ch[e][k], cl[e][k]);
      split2(hv[2 * k], hv[2 * k + 1], hh[k], hl[k]);
    }
    issue_x(cv, hv);                                            // the next step's, before this step's MFMAs
    __builtin_amdgcn_sched_barrier(0);
    unsigned lh[4], ll[4], rh[4], rl[4];                        // tile 0's left neighbours, tile 3's right neighbours
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lh[k] = row_from_left(hh[k], ch[3][k]);
      ll[k] = row_from_left(hl[k], cl[3][k]);
      rh[k] = row_from_right(hh[k], ch[0][k]);
      rl[k] = row_from_right(hl[k], cl[0][k]);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int e = 0; e < NT; ++e) {
          const unsigned(&ph)[4] = t == 1 ? ch[e] : t == 0 ? (e == 0 ? lh : ch[e == 0 ? 0 : e - 1]) : (e == 3 ? rh : ch[e == 3 ? 3 : e + 1]);
          const unsigned(&pl)[4] = t == 1 ? cl[e] : t == 0 ? (e == 0 ? ll : cl[e == 0 ? 0 : e - 1]) : (e == 3 ? rl : cl[e == 3 ? 3 : e + 1]);
          const bf16x8 xh = __builtin_bit_cast(bf16x8, ph), xl = __builtin_bit_cast(bf16x8, pl);
          acc[m][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, w[t][m][0], acc[m][e], 0, 0, 0);
          acc[m][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, w[t][m][0], acc[m][e], 0, 0, 0);
          acc[m][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, w[t][m][1], acc[m][e], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
      issue_w(t, w[t]);                                         // the next step's, in place
      __builtin_amdgcn_sched_barrier(0);
    }
    next_step();
  }

  // ------------------------------------------------------------------ epilogue: acc[m][e][r] = channel 16 m + c at pixel
  // X0 + 16 g + 4 r + e: the four tiles' values of one r are four consecutive pixels, one 16-byte store.  The eight
  // (m, r) vectors of the wave tile are finished by the waves of its group in turn.
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(a.out + (long long)b * a.Cout * HW, 0,
                                                                        (int)((unsigned)a.Cout * plane), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias ? a.Cout * 4 : 0, 0x00020000);
  __shared__ f32x4 red[KS > 1 ? 4 * NTILE * 64 : 1];           // [wave][tile][lane], added below in group order
  if constexpr (KS > 1) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int e = 0; e < NT; ++e) red[(wave * NTILE + m * NT + e) * 64 + lane] = acc[m][e];
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = m * 16 + c;
    const float bv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_b, (unsigned)co * 4u, 0, 0));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (KS > 1 && (m * 4 + r) % KS != q) continue;            // (wave-uniform)
      f32x4 o;
#pragma unroll
      for (int e = 0; e < NT; ++e) {
        float sum = acc[m][e][r];
        if constexpr (KS > 1) {
          sum = red[((grp * KS + 0) * NTILE + m * NT + e) * 64 + lane][r];
#pragma unroll
          for (int k = 1; k < KS; ++k) sum += red[((grp * KS + k) * NTILE + m * NT + e) * 64 + lane][r];
        }
        o[e] = sum + bv;
      }
      const int xo = X0 + 16 * g + 4 * r;
      const bool ok = T < a.ntiles4 && co < a.Cout && xo < W;
      const unsigned off = ((unsigned)co * (unsigned)HW + (unsigned)(ty * W + xo)) * 4u;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_o, ok ? off : OOB, 0, 0);
    }
  }
}

// The K split conv_mfma.hip's dispatch picks for a 3x3 / stride 1 float32 launch to <= 32 channels (conv_dispatch,
// taps = 9): the sums of a wave group are what the bits depend on, the tile shape is not (every form with KS = 1 is the
// same sum).
int staged_ks(int Cin, int Cout, int H, int W, int B) {
  const int nchunk = (Cin + KC - 1) / KC;
  const long long tiles_x = (W + 31) / 32;
  auto wgs = [&](int mt, int th) { return tiles_x * ((H + th - 1) / th) * B * ((Cout + 16 * mt - 1) / (16 * mt)); };
  if (wgs(2, 16) >= 448) return 1;
  if (wgs(2, 8) >= 320) return 1;
  if (wgs(2, 4) < 384 && nchunk >= 8) return 4;
  if (wgs(2, 4) < 768 && nchunk >= 4) return 2;
  return 1;
}

// 16-pixel tiles per wave (never a function of the batch), from the probe at the three offset-convolution shapes of
// DLA-34: one on maps too small to give every CU a workgroup otherwise (32 x 64: 128 workgroups of four K
// groups); from 64 x 128 pixels on, four -- the row form -- where the width is a multiple of 4, else two (the better
// tap form at 64 x 128, 13.6 us against 16.9; widths off the 4-pixel grid themselves were not measured and are not routed).
int pick_nt(int H, int W) {
  if ((long long)H * W < 8192) return 1;
  return (W & 3) == 0 ? 4 : 2;
}

bool shape_ok(int Cin, int Cout, int H, int W) {
  if (Cin < 1 || Cout < 1 || Cout > 16 * MT || H < 1 || W < 1) return false;
  const long long HW = (long long)H * W;
  // 32-bit byte offsets within an image, also for the channels a ragged last chunk reads past it, also with OOB's 2^31 added
  if ((Cin + 2ll * KC) * HW * 4 >= (1ll << 31) || Cin >= (1 << 20)) return false;
  return true;
}

}  // namespace

int cp_conv3x3_stream_supported(int32_t Cin, int32_t Cout, int32_t H, int32_t W) { return shape_ok(Cin, Cout, H, W) ? 1 : 0; }

int cp_conv3x3_stream_form(int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t B) {
  return pick_nt(H, W) << 8 | staged_ks(Cin, Cout, H, W, B);
}

// nt / ks: the tile form (16-pixel tiles per wave 1 | 2 | 4, wave groups per tile 1 | 2 | 4), or 0 / 0 for the form of
// cp_conv3x3_stream_form -- the one that gives cp_conv_mfma_forward's bits; tests and probes force the others
int cp_conv3x3_stream_forward_form(const float* x, const void* wperm, const float* bias, const float* residual, float* out,
                                   int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t relu, int32_t nt,
                                   int32_t ks, void* stream) {
  CP_CHECK_ARG(x && wperm && out && B >= 1 && Cin >= 1 && H >= 1 && W >= 1 && Cout >= 1);
  if (!shape_ok(Cin, Cout, H, W) || B > 65535 || residual || relu) return CP_EUNSUPPORTED;
  Stream3Args a;
  a.x = x;
  a.wp = (const bf16x8*)wperm;
  a.bias = bias;
  a.out = out;
  a.Cin = Cin;
  a.Cout = Cout;
  a.H = H;
  a.W = W;
  a.nchunk = (Cin + KC - 1) / KC;
  a.tpr = (W + 15) / 16;
  a.ntiles = H * a.tpr;
  a.vec = (W & 3) == 0 && (reinterpret_cast<unsigned long long>(out) & 15) == 0;
  a.tpr4 = (W + 63) / 64;
  a.ntiles4 = H * a.tpr4;
  if (nt == 0 && ks == 0) {
    nt = pick_nt(H, W);
    ks = staged_ks(Cin, Cout, H, W, B);
  }
  if ((nt != 1 && nt != 2 && nt != 4) || (ks != 1 && ks != 2 && ks != 4)) return CP_EINVAL;
  const auto launch = [&](auto kernel) {
    const unsigned npg = (unsigned)((a.ntiles + nt - 1) / nt), pgw = 4 / ks;       // wave tiles; of them per workgroup
    hipLaunchKernelGGL(kernel, dim3((npg + pgw - 1) / pgw, B), dim3(256), 0, (hipStream_t)stream, a);
  };
  if (nt == 4 && a.vec) {                  // four interleaved tiles per wave: the row form where the width allows it
    const auto launch4 = [&](auto kernel) {
      const unsigned pgw = 4 / ks;
      hipLaunchKernelGGL(kernel, dim3(((unsigned)a.ntiles4 + pgw - 1) / pgw, B), dim3(256), 0, (hipStream_t)stream, a);
    };
    if (ks == 1) launch4(conv3x3_stream_row4_kernel<1>);
    else if (ks == 2) launch4(conv3x3_stream_row4_kernel<2>);
    else launch4(conv3x3_stream_row4_kernel<4>);
  } else if (nt == 4) {
    if (ks == 1) launch(conv3x3_stream_kernel<4, 1>);
    else if (ks == 2) launch(conv3x3_stream_kernel<4, 2>);
    else launch(conv3x3_stream_kernel<4, 4>);
  } else if (nt == 2) {
    if (ks == 1) launch(conv3x3_stream_kernel<2, 1>);
    else if (ks == 2) launch(conv3x3_stream_kernel<2, 2>);
    else launch(conv3x3_stream_kernel<2, 4>);
  } else {
    if (ks == 1) launch(conv3x3_stream_kernel<1, 1>);
    else if (ks == 2) launch(conv3x3_stream_kernel<1, 2>);
    else launch(conv3x3_stream_kernel<1, 4>);
  }
  return cp_launch_status();
}

int cp_conv3x3_stream_forward(const float* x, const void* wperm, const float* bias, const float* residual, float* out,
                              int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t relu, void* stream) {
  return cp_conv3x3_stream_forward_form(x, wperm, bias, residual, out, B, Cin, H, W, Cout, relu, 0, 0, stream);
}
