// Fused fp32 scaled-dot-product attention for head dim 128 on the bf16 matrix pipes of gfx950:
// the contract, the arithmetic and the orientation of attention.hip (read its header first;
// the shared pieces are attention_common.h), re-derived for rows twice as wide.
//
// As at head dim 64, a workgroup of 4 waves owns 128 rows of one (batch, head), a wave 32 of
// them as the MFMA's B operand in registers, and the other sequence is walked in blocks of 32
// through a two-buffer LDS ring of KC and permuted-TR images; the 32 x 32 tile
// walked row x owned row  never leaves registers between the two GEMMs.  What changes:
//   * an owned row is 8 k-steps of fragments ([8][P] bf16x8, 96 VGPRs per operand at
//     'highest'), the first GEMM 8 k-steps, the second 4 d tiles into floatx16[4];
//   * an image plane of a 32-row block is 8 KiB;
//   * a staging thread (128 per tensor) owns 4 rows x 8 d: two 16-byte loads per row (a
//     quarter-wave reads a row's 512 bytes), one whole 16-byte KC cell per row, and, after the
//     4 x 4 register transposes, eight 8-byte row quads into TR.
//
// LDS images of a 32-row x 128-d block, bf16, one per plane, in 16-byte cells of 8 elements:
//   KC  cell 32 j + (row ^ j), j = d / 8 in 0..15: A fragments with m = row, k = d.  A
//       fragment read (k-step s, half h: j = 2 s + h) is 32 consecutive cells permuted among
//       themselves; a staging store's quarter-wave (one row, j = 0..15) lands in 16 cells that
//       differ mod 16, since  row ^ j  runs through 16 values with distinct low four bits.
//       (The 2 j of head dim 64 would repeat every 8 groups.)
//   TR  cell 128 (2 u + hh) + (d ^ (d / 8 & 7)), elements e: row = 16 u + 8 (e >> 2) + 4 hh +
//       (e & 3): A fragments with m = d, k = row in accumulator-register order.  The xor moves
//       a cell within its aligned group of 8, so a fragment read (32 consecutive d) stays 32
//       consecutive cells permuted; on the store side a thread's d is 8 j + c, cell
//       8 j + (c ^ (j & 7)), so the 16 threads of a row quad spread over all 8 cells mod 8
//       where the plain map would put them all into one.  The staging thread map puts the two
//       8-row halves (e >> 2) into one half-wave, so a half-wave's 256 bytes use both halves
//       of every cell.
//
// The key-owning pass is two kernels, dV and dK.  The fused dK / dV kernel of head dim 64
// stages Q and dO each as KC and TR: 192 KiB double-buffered at 'highest', over the CU's 160,
// and it would hold 192 VGPRs of K / V fragments next to 128 of accumulators.  Split,
//   * the dV kernel owns K, stages Q as KC and dO as TR (96 KiB), recomputes P and
//     accumulates dV: the forward's structure with the saved lse in place of the online
//     softmax;
//   * the dK kernel owns K and V, stages Q as KC and TR and dO as KC (144 KiB), recomputes P
//     and dP and accumulates dK: the dQ kernel with the roles of the sequences exchanged --
//     one template, attention128_grad_kernel, is both.
// That is eight GEMM units against seven (S is formed three times in the backward), and every
// kernel keeps the double-buffered one-barrier stage and 64 accumulator registers.  A
// single-buffered fused kernel would save the eighth unit and expose every stage's global
// latency to all four waves; one image read through the transposing LDS loads would need the
// loads' element order shown equal to the accumulator-register order, which nothing here has
// established.  The cost of the choice is measured in profiles/r18/attention128/README.md.
//
// delta is the diagonal of O dO^T from the six products over the same 8 k-steps, in the order
// of dP, so dP - delta cancels to the bit on one-hot rows.
//
// q, k, v, dO are [B, H, T, 128] views: last stride 1, the others multiples of 4 elements,
// 16-byte aligned base, span below 2 GiB.  O and the gradients are [B, T, H, 128] memory.

#include "attention_common.h"

namespace tgpipe {

namespace {

using namespace attn;

constexpr int kD = 128;                  // head dim
constexpr int kSteps = kD / 16;          // k-steps of a GEMM over d
constexpr int kDt = kD / 32;             // 32-wide d tiles of an output row
constexpr int kPlane = kBlk * kD;        // bf16 per plane of an image
constexpr int kRowPad = kD + 4;          // epilogue rows in LDS, floats

__device__ __forceinline__ int kc_off(int j, int row) { return (j * kBlk + (row ^ j)) * 8; }
__device__ __forceinline__ int tr_off(int slot, int d) {
  return (slot * kD + (d ^ ((d >> 3) & 7))) * 8;
}

// ---- staging: thread u of the 128 of an operand owns rows 4 g .. 4 g + 3, d 8 j .. 8 j + 7.
// g = 4 (u >> 6) + 2 (u >> 4 & 1) + (u >> 5 & 1): a half-wave holds both 8-row halves of a TR
// slot (see the header)
struct Stage {
  floatx4 v[4][2];
  int g, j;

  __device__ __forceinline__ void init(int u) {
    j = u & 15;
    g = 4 * (u >> 6) + 2 * ((u >> 4) & 1) + ((u >> 5) & 1);
  }

  __device__ __forceinline__ void load(const Rows& t, int row0, int T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row0 + 4 * g + i;
      const uint32_t off = t.base + static_cast<uint32_t>(r) * t.pitch + 32u * j;
      v[i][0] = bload4(t.rs, r < T ? off : kOOB);
      v[i][1] = bload4(t.rs, r < T ? off + 16u : kOOB);
    }
  }

  template <int LV>
  __device__ __forceinline__ void store_kc(__bf16* img) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x8 pl[3 - LV];
      split<LV, 8>([&](int e) { return v[i][e >> 2][e & 3]; }, pl);
      __bf16* p = img + kc_off(j, 4 * g + i);
#pragma unroll
      for (int k = 0; k < 3 - LV; ++k) *reinterpret_cast<bf16x8*>(p + k * kPlane) = pl[k];
    }
  }

  // row 4 g + i = 16 u + 8 cc + 4 hh + i: slot 2 u + hh, elements 4 cc + i of d's cell
  template <int LV>
  __device__ __forceinline__ void store_tr(__bf16* img) const {
    const int slot = 2 * (g >> 2) + (g & 1), cc = (g >> 1) & 1;
    __bf16* base = img + (slot * kD + 8 * j) * 8 + 4 * cc;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      bf16x4 pl[3 - LV];
      split<LV, 4>([&](int e) { return v[e][c >> 2][c & 3]; }, pl);
      __bf16* p = base + (c ^ (j & 7)) * 8;  // tr_off(slot, 8 j + c)
#pragma unroll
      for (int k = 0; k < 3 - LV; ++k) *reinterpret_cast<bf16x4*>(p + k * kPlane) = pl[k];
    }
  }
};

// The B fragments of an owned row (n = lane & 31, k = d): 8 k-steps of the first 3 - LV
// planes, straight from memory; a row >= T is 0.
template <int LV>
__device__ __forceinline__ void load_owned(const Rows& t, int row, int T, int h,
                                           bf16x8 (&f)[kSteps][3 - LV]) {
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const uint32_t off =
        row < T ? t.base + static_cast<uint32_t>(row) * t.pitch + 4u * (16 * s + 8 * h) : kOOB;
    const floatx4 a = bload4(t.rs, off), b = bload4(t.rs, row < T ? off + 16u : kOOB);
    split<LV, 8>([&](int e) { return e < 4 ? a[e] : b[e - 4]; }, f[s]);
  }
}

// acc[walked][owned] += sum_d A(walked, d) B(owned, d): A from a KC image.  SWAP: the pairs
// name (B's plane, A's plane) -- the order of the same product with the operands' roles
// exchanged.
template <int LV, bool SWAP = false>
__device__ __forceinline__ void gemm_kc(floatx16& acc, const __bf16* img,
                                        const bf16x8 (&b)[kSteps][3 - LV], int h, int l32) {
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    bf16x8 a[3 - LV];
#pragma unroll
    for (int p = 0; p < 3 - LV; ++p)
      a[p] = *reinterpret_cast<const bf16x8*>(img + p * kPlane + kc_off(2 * s + h, l32));
#pragma unroll
    for (int t = first_pair(LV); t < 6; ++t)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kPairs[t][SWAP ? 1 : 0]],
                                                    b[s][kPairs[t][SWAP ? 0 : 1]], acc, 0, 0, 0);
  }
}

// acc[dt][d][owned] += sum_walked X^T(d, walked) tile(walked, owned): A from a TR image, B the
// split tile (b[u]: registers 8 u .. 8 u + 7)
template <int LV>
__device__ __forceinline__ void gemm_tr(floatx16 (&acc)[kDt], const __bf16* img,
                                        const bf16x8 (&b)[2][3 - LV], int h, int l32) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) {
      bf16x8 a[3 - LV];
#pragma unroll
      for (int p = 0; p < 3 - LV; ++p)
        a[p] = *reinterpret_cast<const bf16x8*>(img + p * kPlane +
                                                tr_off(2 * u + h, 32 * dt + l32));
#pragma unroll
      for (int t = first_pair(LV); t < 6; ++t)
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kPairs[t][0]], b[u][kPairs[t][1]],
                                                          acc[dt], 0, 0, 0);
    }
}

// acc[dt][d][owned] * mul(owned) -> out[owned][d], rows of `pitch` floats: through the wave's
// 32 x 128 LDS tile to coalesced 512-byte row stores.  Every wave of the workgroup calls it
// (two barriers); `lds` must be free of staging traffic.
__device__ __forceinline__ void store_owned(float* lds, const floatx16 (&acc)[kDt], float mul,
                                            float* out, int64_t pitch, int row0, int T, int wave,
                                            int lane) {
  const int h = lane >> 5, l32 = lane & 31;
  float* tile = lds + wave * 32 * kRowPad;
  __syncthreads();
#pragma unroll
  for (int dt = 0; dt < kDt; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<floatx4*>(tile + l32 * kRowPad + 32 * dt + 8 * j + 4 * h) =
          floatx4{acc[dt][4 * j] * mul, acc[dt][4 * j + 1] * mul, acc[dt][4 * j + 2] * mul,
                  acc[dt][4 * j + 3] * mul};
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int idx = it * 64 + lane, row = idx >> 5, qd = idx & 31;
    if (row0 + row < T)
      *reinterpret_cast<floatx4*>(out + (row0 + row) * pitch + 4 * qd) =
          *reinterpret_cast<const floatx4*>(tile + row * kRowPad + 4 * qd);
  }
}

// the ring of `images` images per stage with the walked block's 2 x 32 statistics behind it,
// or the four waves' epilogue tiles
constexpr int lds_bytes(int images, int lv) {
  const int ring = 2 * images * (3 - lv) * kPlane * 2 + 2 * 2 * kBlk * 4;
  const int epi = 4 * 32 * kRowPad * 4;
  return ring > epi ? ring : epi;
}

// ---- forward ---------------------------------------------------------------------------------
// One workgroup per (query block of 128, b, h).  Images per stage: K as KC, V as TR.
template <int LV, bool CAUSAL>
__global__ __launch_bounds__(kThreads) void attention128_fwd_kernel(AttnArgs p) {
  constexpr int P = 3 - LV, kImg = P * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[lds_bytes(2, LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<CAUSAL, true>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T, q0 = w.rb * kOwn;
  const int qw = q0 + 32 * wave, my = qw + l32;
  const Rows Q = rows_of(p.q, b, hd), K = rows_of(p.k, b, hd), V = rows_of(p.v, b, hd);

  bf16x8 qf[kSteps][P];
  load_owned<LV>(Q, my, T, h, qf);
  floatx16 o[kDt];
#pragma unroll
  for (int dt = 0; dt < kDt; ++dt) zero(o[dt]);
  float m = -INFINITY, l = 0.f;

  const int blocks = CAUSAL ? min(q0 + kOwn - 1, T - 1) / kBlk + 1 : (T + kBlk - 1) / kBlk;
  const bool upper = tid >= kThreads / 2;  // stages V; the lower half K
  Stage st;
  st.init(tid & 127);
  auto kimg = [&](int buf) { return lds + buf * 2 * kImg; };
  auto vimg = [&](int buf) { return lds + buf * 2 * kImg + kImg; };
  auto load = [&](int kb) { st.load(upper ? V : K, kb * kBlk, T); };
  auto store = [&](int buf) {
    if (upper) st.template store_tr<LV>(vimg(buf));
    else st.template store_kc<LV>(kimg(buf));
  };

  load(0);
  store(0);
  __syncthreads();
  for (int kb = 0; kb < blocks; ++kb) {
    const int buf = kb & 1, k0 = kb * kBlk;
    if (kb + 1 < blocks) load(kb + 1);
    if (!CAUSAL || k0 <= qw + 31) {  // (wave-uniform) not wholly above the wave's diagonal
      floatx16 s;
      zero(s);
      gemm_kc<LV>(s, kimg(buf), qf, h, l32);
      const bool edge = k0 + kBlk > T || (CAUSAL && k0 + kBlk - 1 > qw);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + walked_row(r, h);
        s[r] *= p.scale;
        if (edge && (key >= T || (CAUSAL && key > my))) s[r] = -INFINITY;
        mx = fmaxf(mx, s[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      // (every row sees key k0 of its first block, so m_new is finite)
      const float m_new = fmaxf(m, mx), alpha = expf(m - m_new);
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = expf(s[r] - m_new);
        sum += s[r];
      }
      sum += __shfl_xor(sum, 32);
      l = l * alpha + sum;
      m = m_new;
#pragma unroll
      for (int dt = 0; dt < kDt; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
      bf16x8 pf[2][P];
      split_tile<LV>(s, pf);
      gemm_tr<LV>(o, vimg(buf), pf, h, l32);
    }
    if (kb + 1 < blocks) store(buf ^ 1);
    __syncthreads();
  }

  float* out = p.o + (static_cast<int64_t>(b) * T * p.H + hd) * kD;
  store_owned(reinterpret_cast<float*>(lds_raw), o, 1.f / l, out, static_cast<int64_t>(p.H) * kD,
              qw, T, wave, lane);
  if (h == 0 && my < T) p.lse[static_cast<int64_t>(w.bh) * T + my] = m + logf(l);
}

// ---- delta[b][h][t] = sum_d dO[b][h][t][d] O[b][t][h][d] ---------------------------------------
// The diagonal of the 32 x 32 tile O dO^T of a wave's 32 rows, formed exactly as the backward
// kernels form dP = V dO^T (A the KC image, B the row fragments, the same products over the
// same 8 k-steps in the same order).  Always the six products: delta is an fp32 quantity at
// every level.  A wave's O image is 24 KiB.
__global__ __launch_bounds__(kThreads) void attention128_delta_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[4 * 3 * kPlane];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<false, false>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T;
  const int rw = w.rb * kOwn + 32 * wave, my = rw + l32;
  __bf16* img = lds + wave * 3 * kPlane;
  const float* o = p.o + (static_cast<int64_t>(b) * T * p.H + hd) * kD;
  const int64_t pitch = static_cast<int64_t>(p.H) * kD;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int idx = it * 64 + lane, row = idx >> 4, j = idx & 15;
    floatx4 v[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
    if (rw + row < T) {
      const float* src = o + (rw + row) * pitch + 8 * j;
      v[0] = *reinterpret_cast<const floatx4*>(src);
      v[1] = *reinterpret_cast<const floatx4*>(src + 4);
    }
    bf16x8 pl[3];
    split<0, 8>([&](int e) { return v[e >> 2][e & 3]; }, pl);
    __bf16* at = img + kc_off(j, row);
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<bf16x8*>(at + k * kPlane) = pl[k];
  }
  bf16x8 gf[kSteps][3];
  load_owned<0>(rows_of(p.dout, b, hd), my, T, h, gf);
  __syncthreads();
  floatx16 tile;
  zero(tile);
  gemm_kc<0>(tile, img, gf, h, l32);
  // row l32 of column l32 is register (l32 & 3) + 4 (l32 >> 3) of the half (l32 >> 2) & 1
  float d = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (walked_row(r, h) == l32) d = tile[r];
  if (((l32 >> 2) & 1) == h && my < T) p.delta[static_cast<int64_t>(w.bh) * T + my] = d;
}

// ---- dQ (KEYS false) and dK (KEYS true) -------------------------------------------------------
// dQ owns queries (Q and dO fragments) and walks keys: K as KC and TR, V as KC.  dK owns keys
// (K and V fragments) and walks queries: Q as KC and TR, dO as KC, with the block's lse and
// delta as 2 x 32 floats behind the ring.  Either way  tile[walked][owned]: S from the first
// pair, dP from the second, dS = P (dP - delta), and the owned gradient  += X_tr dS  with X
// the walked tensor of the first pair.  With keys owned the operands' roles in S and dP are
// exchanged, and so are the pairs (SWAP): S rounds as the forward's and dP as delta.
template <int LV, bool CAUSAL, bool KEYS>
__global__ __launch_bounds__(kThreads) void attention128_grad_kernel(AttnArgs p) {
  constexpr int P = 3 - LV, kImg = P * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[lds_bytes(3, LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  float* stats = reinterpret_cast<float*>(lds + 2 * 3 * kImg);  // KEYS: [buf][lse, delta][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<CAUSAL, !KEYS>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T, r0 = w.rb * kOwn;
  const int rw = r0 + 32 * wave, my = rw + l32;
  const Rows X = rows_of(KEYS ? p.q : p.k, b, hd), Y = rows_of(KEYS ? p.dout : p.v, b, hd);

  bf16x8 xf[kSteps][P], yf[kSteps][P];  // the owned partners of X and Y
  load_owned<LV>(rows_of(KEYS ? p.k : p.q, b, hd), my, T, h, xf);
  load_owned<LV>(rows_of(KEYS ? p.v : p.dout, b, hd), my, T, h, yf);
  float lse = 0.f, delta = 0.f;  // queries owned: the lane's own
  if (!KEYS && my < T) {
    lse = p.lse[static_cast<int64_t>(w.bh) * T + my];
    delta = p.delta[static_cast<int64_t>(w.bh) * T + my];
  }
  floatx16 acc[kDt];
#pragma unroll
  for (int dt = 0; dt < kDt; ++dt) zero(acc[dt]);

  // causal: queries walk the keys up to their block's last; keys walk the queries from their
  // block's first
  const int first = KEYS && CAUSAL ? r0 / kBlk : 0;
  const int blocks =
      !KEYS && CAUSAL ? min(r0 + kOwn - 1, T - 1) / kBlk + 1 : (T + kBlk - 1) / kBlk;
  const bool upper = tid >= kThreads / 2;  // stages Y; the lower half X
  Stage st;
  st.init(tid & 127);
  float stat = 0.f;  // KEYS, threads 0-31: a walked query's lse; 32-63: its delta
  const float* stat_src = (tid < 32 ? p.lse : p.delta) + static_cast<int64_t>(w.bh) * T;
  auto xkc = [&](int buf) { return lds + buf * 3 * kImg; };
  auto xtr = [&](int buf) { return lds + buf * 3 * kImg + kImg; };
  auto ykc = [&](int buf) { return lds + buf * 3 * kImg + 2 * kImg; };
  auto load = [&](int wb) {
    st.load(upper ? Y : X, wb * kBlk, T);
    if constexpr (KEYS) {
      const int q = wb * kBlk + (tid & 31);
      if (tid < 64) stat = q < T ? stat_src[q] : 0.f;
    }
  };
  auto store = [&](int buf) {
    if (upper) {
      st.template store_kc<LV>(ykc(buf));
    } else {
      st.template store_kc<LV>(xkc(buf));
      st.template store_tr<LV>(xtr(buf));
    }
    if constexpr (KEYS)
      if (tid < 64) stats[buf * 64 + tid] = stat;
  };

  if (first < blocks) {
    load(first);
    store(first & 1);
  }
  __syncthreads();
  for (int wb = first; wb < blocks; ++wb) {
    const int buf = wb & 1, w0 = wb * kBlk;
    if (wb + 1 < blocks) load(wb + 1);
    // (wave-uniform) the block is not wholly on the masked side of the wave's diagonal
    if (!CAUSAL || (KEYS ? w0 + kBlk - 1 >= rw : w0 <= rw + 31)) {
      floatx16 s, dp;
      zero(s);
      zero(dp);
      gemm_kc<LV, KEYS>(s, xkc(buf), xf, h, l32);
      gemm_kc<LV, KEYS>(dp, ykc(buf), yf, h, l32);
      const bool edge = w0 + kBlk > T || (KEYS && rw + 32 > T) ||
                        (CAUSAL && (KEYS ? rw + 31 > w0 : w0 + kBlk - 1 > rw));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        floatx4 lse4 = floatx4{lse, lse, lse, lse}, del4 = floatx4{delta, delta, delta, delta};
        if constexpr (KEYS) {
          lse4 = *reinterpret_cast<const floatx4*>(stats + buf * 64 + 8 * j + 4 * h);
          del4 = *reinterpret_cast<const floatx4*>(stats + buf * 64 + 32 + 8 * j + 4 * h);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * j + i, x = w0 + 8 * j + 4 * h + i;  // x: the walked row of r
          const bool off =
              edge && (x >= T || (KEYS ? my >= T || (CAUSAL && my > x) : CAUSAL && x > my));
          const float pr = off ? 0.f : expf(s[r] * p.scale - lse4[i]);
          s[r] = pr * (dp[r] - del4[i]);
        }
      }
      bf16x8 df[2][P];
      split_tile<LV>(s, df);
      gemm_tr<LV>(acc, xtr(buf), df, h, l32);
    }
    if (wb + 1 < blocks) store(buf ^ 1);
    __syncthreads();
  }

  float* out = (KEYS ? p.dk : p.dq) + (static_cast<int64_t>(b) * T * p.H + hd) * kD;
  store_owned(reinterpret_cast<float*>(lds_raw), acc, p.scale, out,
              static_cast<int64_t>(p.H) * kD, rw, T, wave, lane);
}

// ---- dV: owns keys (K fragments), walks queries.  Images per stage: Q as KC, dO as TR; the
// block's lse rides along behind the ring ------------------------------------------------------
template <int LV, bool CAUSAL>
__global__ __launch_bounds__(kThreads) void attention128_dv_kernel(AttnArgs p) {
  constexpr int P = 3 - LV, kImg = P * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[lds_bytes(2, LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  float* stats = reinterpret_cast<float*>(lds + 2 * 2 * kImg);  // [buf][lse][32] (64 apart)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<CAUSAL, false>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T;
  const int k0 = w.rb * kOwn, kw = k0 + 32 * wave, my = kw + l32;
  const Rows Q = rows_of(p.q, b, hd), G = rows_of(p.dout, b, hd);

  bf16x8 kf[kSteps][P];
  load_owned<LV>(rows_of(p.k, b, hd), my, T, h, kf);
  floatx16 dv[kDt];
#pragma unroll
  for (int dt = 0; dt < kDt; ++dt) zero(dv[dt]);

  // causal: the first query block that reaches the workgroup's keys
  const int first = CAUSAL ? k0 / kBlk : 0, blocks = (T + kBlk - 1) / kBlk;
  const bool upper = tid >= kThreads / 2;  // stages dO; the lower half Q
  Stage st;
  st.init(tid & 127);
  float stat = 0.f;  // threads 0-31: a query's lse
  const float* lse_src = p.lse + static_cast<int64_t>(w.bh) * T;
  auto qimg = [&](int buf) { return lds + buf * 2 * kImg; };
  auto gimg = [&](int buf) { return lds + buf * 2 * kImg + kImg; };
  auto load = [&](int qb) {
    st.load(upper ? G : Q, qb * kBlk, T);
    const int q = qb * kBlk + tid;
    if (tid < 32) stat = q < T ? lse_src[q] : 0.f;
  };
  auto store = [&](int buf) {
    if (upper) st.template store_tr<LV>(gimg(buf));
    else st.template store_kc<LV>(qimg(buf));
    if (tid < 32) stats[buf * 64 + tid] = stat;
  };

  if (first < blocks) {
    load(first);
    store(first & 1);
  }
  __syncthreads();
  for (int qb = first; qb < blocks; ++qb) {
    const int buf = qb & 1, q0 = qb * kBlk;
    if (qb + 1 < blocks) load(qb + 1);
    if (!CAUSAL || q0 + kBlk - 1 >= kw) {  // (wave-uniform) some query reaches the wave's keys
      floatx16 s;
      zero(s);
      gemm_kc<LV, true>(s, qimg(buf), kf, h, l32);  // (pairs exchanged: S as the forward's)
      const bool edge = q0 + kBlk > T || kw + 32 > T || (CAUSAL && kw + 31 > q0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const floatx4 lse4 = *reinterpret_cast<const floatx4*>(stats + buf * 64 + 8 * j + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * j + i, q = q0 + 8 * j + 4 * h + i;
          const bool off = edge && (q >= T || my >= T || (CAUSAL && my > q));
          s[r] = off ? 0.f : expf(s[r] * p.scale - lse4[i]);
        }
      }
      bf16x8 pf[2][P];
      split_tile<LV>(s, pf);
      gemm_tr<LV>(dv, gimg(buf), pf, h, l32);
    }
    if (qb + 1 < blocks) store(buf ^ 1);
    __syncthreads();
  }

  float* out = p.dv + (static_cast<int64_t>(b) * T * p.H + hd) * kD;
  store_owned(reinterpret_cast<float*>(lds_raw), dv, 1.f, out, static_cast<int64_t>(p.H) * kD,
              kw, T, wave, lane);
}

}  // namespace

void launch_attention128_forward(const AttnArgs& a, bool causal, hipStream_t stream) {
  with_instance(causal, [&](auto lv, auto cs) {
    hipLaunchKernelGGL((attention128_fwd_kernel<decltype(lv)::value, decltype(cs)::value>),
                       attn_grid(a), dim3(kThreads), 0, stream, a);
  });
}

// delta, then dV and dK (a workgroup per key block), then dQ (a workgroup per query block)
void launch_attention128_backward(const AttnArgs& a, bool causal, hipStream_t stream) {
  hipLaunchKernelGGL(attention128_delta_kernel, attn_grid(a), dim3(kThreads), 0, stream, a);
  with_instance(causal, [&](auto lv, auto cs) {
    constexpr int LV = decltype(lv)::value;
    constexpr bool CS = decltype(cs)::value;
    hipLaunchKernelGGL((attention128_dv_kernel<LV, CS>), attn_grid(a), dim3(kThreads), 0, stream,
                       a);
    hipLaunchKernelGGL((attention128_grad_kernel<LV, CS, true>), attn_grid(a), dim3(kThreads), 0,
                       stream, a);
    hipLaunchKernelGGL((attention128_grad_kernel<LV, CS, false>), attn_grid(a), dim3(kThreads),
                       0, stream, a);
  });
}

}  // namespace tgpipe
