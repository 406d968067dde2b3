// Fused fp32 scaled-dot-product attention for head dim 64 on the bf16 matrix pipes of gfx950:
// O = softmax(scale Q K^T [+ causal mask]) V, forward and backward, flash style (no T x T
// tensor in memory), no atomics, nothing the host reads.  The arithmetic is linear.hip's:
// every operand of every GEMM is split exactly into bf16 planes hi / mid / lo (split1), a
// product is the level's partial products, small parts first (kPairs), on
// v_mfma_f32_32x32x16_bf16 with f32 accumulators; the level of conv_precision picks the
// instance and a reduced level never forms the planes it drops.  P is in [0, 1] in fp32 and is
// split like any other operand.
//
// Orientation.  A workgroup of 4 waves owns 128 rows of one (batch, head) -- queries in the
// forward and the dQ kernel, keys in the dK / dV kernel -- and walks the other sequence in
// blocks of 32 through a two-buffer LDS ring.  A wave owns 32 of the rows for the whole pass:
// their Q (or K, V, dO) fragments stay in registers as the MFMA's B operand, so in the 32 x 32
// score tile  walked row x owned row  an owned row is a lane (lane & 31) and the walked rows
// are the lane's 16 registers, (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Hence
//   * the online softmax's row max / row sum are reductions over a lane's registers plus one
//     exchange with lane ^ 32, and the rescale of the running output a per-lane scalar;
//   * registers 0-7 and 8-15 of a lane are, once split, two B fragments of the second GEMM
//     out^T[d][owned] = sum_walked X^T[d][walked] tile[walked][owned] if its reduction index
//     runs over the walked rows in that register order.  A sum does not care about order, so
//     X (V; dO and Q; K) is staged into LDS transposed with its rows permuted to match (the
//     TR image); an A fragment is then one ds_read_b128.  The tile never leaves registers.
//
// LDS images of a 32-row x 64-d block, bf16, one per plane:
//   KC  [d / 8][row ^ 2 (d / 8)][8 d]: A fragments with m = row, k = d (linear.hip's image);
//   TR  [2 u + h][d][8 e], row = 16 u + 8 (e >> 2) + 4 h + (e & 3): A fragments with m = d,
//       k = row in accumulator-register order.
// Both are written from the same registers: a staging thread loads a 4-row x 4-d block (16
// bytes per row; a wave reads runs of 256 bytes), stores four d quads into KC and, after the
// 4 x 4 register transpose of linear.hip's KR staging, four row quads into TR.  The lower
// half of the workgroup stages one tensor, the upper half the other.  The next block's global
// loads are issued ahead of the stage's MFMAs, split and stored behind them; one barrier per
// stage.
//
// Tails: rows >= T read 0 through raw buffer loads at an offset past the tensor (kOOB) and
// are masked to -inf (P = 0) before the max.  Causal: blocks wholly above the diagonal are
// never staged (workgroup) or multiplied (wave); only blocks that cross it are masked.
//
// Backward: delta = rowsum(dO . O) first (from the products and in the order of dP); then one
// kernel per ownership, so nothing is accumulated atomically.  The dK / dV kernel owns keys
// and recomputes S[query][key] (A = Q, B = K), the dQ kernel owns queries and recomputes
// S^T[key][query] (A = K, B = Q); both form
// P = exp(scale S - lse), dP from V and dO, dS = P (dP - delta).  Seven GEMM units against
// the five of an atomic dQ: the price of bitwise reproducibility, as in the split-K
// reductions.
//
// q, k, v, dO are [B, H, T, 64] views: last stride 1, the others multiples of 4 elements,
// 16-byte aligned base, span below 2 GiB.  O and the gradients are [B, T, H, 64] memory.

// The arithmetic, the operand views, the grid order and the level dispatch are shared with the
// head-dim-128 kernels of attention128.hip through attention_common.h.

#include "attention_common.h"

namespace tgpipe {

namespace {

using namespace attn;

constexpr int kD = 64;                   // head dim
constexpr int kPlane = kBlk * kD;        // bf16 per plane of an image
constexpr int kRowPad = kD + 4;          // epilogue rows in LDS, floats

__device__ __forceinline__ int kc_off(int j, int row) { return (j * kBlk + (row ^ (2 * j))) * 8; }

// ---- staging: thread u of the 128 of an operand owns rows 4 g .. 4 g + 3, d 4 dq .. 4 dq + 3
struct Stage {
  floatx4 v[4];
  int g, dq;

  __device__ __forceinline__ void init(int u) {
    dq = u & 15;
    g = u >> 4;
  }

  __device__ __forceinline__ void load(const Rows& t, int row0, int T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row0 + 4 * g + i;
      v[i] = bload4(t.rs, r < T ? t.base + static_cast<uint32_t>(r) * t.pitch + 16u * dq : kOOB);
    }
  }

  template <int LV>
  __device__ __forceinline__ void store_kc(__bf16* img) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 pl[3 - LV];
      split<LV, 4>([&](int e) { return v[i][e]; }, pl);
      __bf16* p = img + kc_off(dq >> 1, 4 * g + i) + 4 * (dq & 1);
#pragma unroll
      for (int k = 0; k < 3 - LV; ++k) *reinterpret_cast<bf16x4*>(p + k * kPlane) = pl[k];
    }
  }

  // row 4 g + i = 16 u + 8 cc + 4 h + i: slot 2 u + h, elements 4 cc + i of d's row
  template <int LV>
  __device__ __forceinline__ void store_tr(__bf16* img) const {
    const int slot = 2 * (g >> 2) + (g & 1), cc = (g >> 1) & 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bf16x4 pl[3 - LV];
      split<LV, 4>([&](int e) { return v[e][c]; }, pl);
      __bf16* p = img + (slot * kD + 4 * dq + c) * 8 + 4 * cc;
#pragma unroll
      for (int k = 0; k < 3 - LV; ++k) *reinterpret_cast<bf16x4*>(p + k * kPlane) = pl[k];
    }
  }
};

// The B fragments of an owned row (n = lane & 31, k = d): 4 k steps of the first 3 - LV
// planes, straight from memory; a row >= T is 0.
template <int LV>
__device__ __forceinline__ void load_owned(const Rows& t, int row, int T, int h,
                                           bf16x8 (&f)[4][3 - LV]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
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
                                        const bf16x8 (&b)[4][3 - LV], int h, int l32) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
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
__device__ __forceinline__ void gemm_tr(floatx16 (&acc)[2], const __bf16* img,
                                        const bf16x8 (&b)[2][3 - LV], int h, int l32) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      bf16x8 a[3 - LV];
#pragma unroll
      for (int p = 0; p < 3 - LV; ++p)
        a[p] = *reinterpret_cast<const bf16x8*>(img + p * kPlane +
                                                ((2 * u + h) * kD + 32 * dt + l32) * 8);
#pragma unroll
      for (int t = first_pair(LV); t < 6; ++t)
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kPairs[t][0]], b[u][kPairs[t][1]],
                                                          acc[dt], 0, 0, 0);
    }
}

// acc[dt][d][owned] * mul(owned) -> out[owned][d], rows of `pitch` floats: through the wave's
// 32 x 64 LDS tile to coalesced 256-byte row stores.  Every wave of the workgroup calls it
// (two barriers); `lds` must be free of staging traffic.
__device__ __forceinline__ void store_owned(float* lds, const floatx16 (&acc)[2], float mul,
                                            float* out, int64_t pitch, int row0, int T, int wave,
                                            int lane) {
  const int h = lane >> 5, l32 = lane & 31;
  float* tile = lds + wave * 32 * kRowPad;
  __syncthreads();
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<floatx4*>(tile + l32 * kRowPad + 32 * dt + 8 * j + 4 * h) =
          floatx4{acc[dt][4 * j] * mul, acc[dt][4 * j + 1] * mul, acc[dt][4 * j + 2] * mul,
                  acc[dt][4 * j + 3] * mul};
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int idx = it * 64 + lane, row = idx >> 4, qd = idx & 15;
    if (row0 + row < T)
      *reinterpret_cast<floatx4*>(out + (row0 + row) * pitch + 4 * qd) =
          *reinterpret_cast<const floatx4*>(tile + row * kRowPad + 4 * qd);
  }
}

constexpr int lds_bytes(int images, int lv) {
  const int ring = 2 * images * (3 - lv) * kPlane * 2 + 2 * 2 * kBlk * 4;
  const int epi = 4 * 32 * kRowPad * 4;
  return ring > epi ? ring : epi;
}

// ---- forward ---------------------------------------------------------------------------------
// One workgroup per (query block of 128, b, h).  Images per stage: K as KC, V as TR.
template <int LV, bool CAUSAL>
__global__ __launch_bounds__(kThreads) void attention_fwd_kernel(AttnArgs p) {
  constexpr int P = 3 - LV, kImg = P * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[lds_bytes(2, LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<CAUSAL, true>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T, q0 = w.rb * kOwn;
  const int qw = q0 + 32 * wave, my = qw + l32;
  const Rows Q = rows_of(p.q, b, hd), K = rows_of(p.k, b, hd), V = rows_of(p.v, b, hd);

  bf16x8 qf[4][P];
  load_owned<LV>(Q, my, T, h, qf);
  floatx16 o[2];
  zero(o[0]);
  zero(o[1]);
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
      for (int dt = 0; dt < 2; ++dt)
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
// kernels form dP = V dO^T (A the KC image, B the row fragments, the same products in the same
// order): where the softmax is one-hot, O is the row of V and dP - delta cancels to the bit,
// as it does in exact arithmetic.  Always the six products: delta is an fp32 quantity at every
// level.
__global__ __launch_bounds__(kThreads) void attention_delta_kernel(AttnArgs p) {
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
    const int idx = it * 64 + lane, row = idx >> 4, dq = idx & 15;
    floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
    if (rw + row < T) v = *reinterpret_cast<const floatx4*>(o + (rw + row) * pitch + 4 * dq);
    bf16x4 pl[3];
    split<0, 4>([&](int e) { return v[e]; }, pl);
    __bf16* at = img + kc_off(dq >> 1, row) + 4 * (dq & 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<bf16x4*>(at + k * kPlane) = pl[k];
  }
  bf16x8 gf[4][3];
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

// ---- dQ: owns queries, walks keys.  Images per stage: K as KC and TR, V as KC ------------------
template <int LV, bool CAUSAL>
__global__ __launch_bounds__(kThreads) void attention_dq_kernel(AttnArgs p) {
  constexpr int P = 3 - LV, kImg = P * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[lds_bytes(3, LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<CAUSAL, true>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T, q0 = w.rb * kOwn;
  const int qw = q0 + 32 * wave, my = qw + l32;
  const Rows Q = rows_of(p.q, b, hd), K = rows_of(p.k, b, hd), V = rows_of(p.v, b, hd),
             G = rows_of(p.dout, b, hd);

  bf16x8 qf[4][P], gf[4][P];
  load_owned<LV>(Q, my, T, h, qf);
  load_owned<LV>(G, my, T, h, gf);
  const int64_t stat = static_cast<int64_t>(w.bh) * T + my;
  const float lse = my < T ? p.lse[stat] : 0.f, delta = my < T ? p.delta[stat] : 0.f;
  floatx16 dq[2];
  zero(dq[0]);
  zero(dq[1]);

  const int blocks = CAUSAL ? min(q0 + kOwn - 1, T - 1) / kBlk + 1 : (T + kBlk - 1) / kBlk;
  const bool upper = tid >= kThreads / 2;  // stages V; the lower half K
  Stage st;
  st.init(tid & 127);
  auto kimg = [&](int buf) { return lds + buf * 3 * kImg; };
  auto ktr = [&](int buf) { return lds + buf * 3 * kImg + kImg; };
  auto vimg = [&](int buf) { return lds + buf * 3 * kImg + 2 * kImg; };
  auto load = [&](int kb) { st.load(upper ? V : K, kb * kBlk, T); };
  auto store = [&](int buf) {
    if (upper) {
      st.template store_kc<LV>(vimg(buf));
    } else {
      st.template store_kc<LV>(kimg(buf));
      st.template store_tr<LV>(ktr(buf));
    }
  };

  load(0);
  store(0);
  __syncthreads();
  for (int kb = 0; kb < blocks; ++kb) {
    const int buf = kb & 1, k0 = kb * kBlk;
    if (kb + 1 < blocks) load(kb + 1);
    if (!CAUSAL || k0 <= qw + 31) {
      floatx16 s, dp;
      zero(s);
      zero(dp);
      gemm_kc<LV>(s, kimg(buf), qf, h, l32);
      gemm_kc<LV>(dp, vimg(buf), gf, h, l32);
      const bool edge = k0 + kBlk > T || (CAUSAL && k0 + kBlk - 1 > qw);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + walked_row(r, h);
        const bool off = edge && (key >= T || (CAUSAL && key > my));
        const float pr = off ? 0.f : expf(s[r] * p.scale - lse);
        s[r] = pr * (dp[r] - delta);
      }
      bf16x8 df[2][P];
      split_tile<LV>(s, df);
      gemm_tr<LV>(dq, ktr(buf), df, h, l32);
    }
    if (kb + 1 < blocks) store(buf ^ 1);
    __syncthreads();
  }

  float* out = p.dq + (static_cast<int64_t>(b) * T * p.H + hd) * kD;
  store_owned(reinterpret_cast<float*>(lds_raw), dq, p.scale, out,
              static_cast<int64_t>(p.H) * kD, qw, T, wave, lane);
}

// ---- dK, dV: owns keys, walks queries.  Images per stage: Q and dO, each as KC and TR; the
// block's lse and delta ride along as 2 x 32 floats behind the ring -----------------------------
template <int LV, bool CAUSAL>
__global__ __launch_bounds__(kThreads) void attention_dkv_kernel(AttnArgs p) {
  constexpr int P = 3 - LV, kImg = P * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[lds_bytes(4, LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
  float* stats = reinterpret_cast<float*>(lds + 2 * 4 * kImg);  // [buf][lse, delta][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const Where w = where<CAUSAL, false>(p);
  const int b = w.bh / p.H, hd = w.bh % p.H, T = p.T;
  const int k0 = w.rb * kOwn, kw = k0 + 32 * wave, my = kw + l32;
  const Rows Q = rows_of(p.q, b, hd), K = rows_of(p.k, b, hd), V = rows_of(p.v, b, hd),
             G = rows_of(p.dout, b, hd);

  bf16x8 kf[4][P], vf[4][P];
  load_owned<LV>(K, my, T, h, kf);
  load_owned<LV>(V, my, T, h, vf);
  floatx16 dk[2], dv[2];
  zero(dk[0]);
  zero(dk[1]);
  zero(dv[0]);
  zero(dv[1]);

  // causal: the first query block that reaches the workgroup's keys
  const int first = CAUSAL ? k0 / kBlk : 0, blocks = (T + kBlk - 1) / kBlk;
  const bool upper = tid >= kThreads / 2;  // stages dO; the lower half Q
  Stage st;
  st.init(tid & 127);
  float stat = 0.f;  // threads 0-31: a query's lse; 32-63: its delta
  const float* stat_src = (tid < 32 ? p.lse : p.delta) + static_cast<int64_t>(w.bh) * T;
  auto img = [&](int buf, int i) { return lds + (buf * 4 + i) * kImg; };  // Q kc, Q tr, dO kc, tr
  auto load = [&](int qb) {
    st.load(upper ? G : Q, qb * kBlk, T);
    const int q = qb * kBlk + (tid & 31);
    if (tid < 64) stat = q < T ? stat_src[q] : 0.f;
  };
  auto store = [&](int buf) {
    st.template store_kc<LV>(img(buf, upper ? 2 : 0));
    st.template store_tr<LV>(img(buf, upper ? 3 : 1));
    if (tid < 64) stats[buf * 64 + tid] = stat;
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
      floatx16 s, dp;
      zero(s);
      zero(dp);
      // (the owned rows are K and V here: the pairs exchanged, so S rounds as the forward's
      // and dP as delta)
      gemm_kc<LV, true>(s, img(buf, 0), kf, h, l32);
      gemm_kc<LV, true>(dp, img(buf, 2), vf, h, l32);
      const bool edge = q0 + kBlk > T || kw + 32 > T || (CAUSAL && kw + 31 > q0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const floatx4 lse4 = *reinterpret_cast<const floatx4*>(stats + buf * 64 + 8 * j + 4 * h);
        const floatx4 del4 =
            *reinterpret_cast<const floatx4*>(stats + buf * 64 + 32 + 8 * j + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * j + i, q = q0 + 8 * j + 4 * h + i;
          const bool off = edge && (q >= T || my >= T || (CAUSAL && my > q));
          const float pr = off ? 0.f : expf(s[r] * p.scale - lse4[i]);
          s[r] = pr;
          dp[r] = pr * (dp[r] - del4[i]);
        }
      }
      bf16x8 pf[2][P];
      split_tile<LV>(s, pf);
      gemm_tr<LV>(dv, img(buf, 3), pf, h, l32);
      split_tile<LV>(dp, pf);
      gemm_tr<LV>(dk, img(buf, 1), pf, h, l32);
    }
    if (qb + 1 < blocks) store(buf ^ 1);
    __syncthreads();
  }

  const int64_t at = (static_cast<int64_t>(b) * T * p.H + hd) * kD, pitch = p.H * kD;
  store_owned(reinterpret_cast<float*>(lds_raw), dk, p.scale, p.dk + at, pitch, kw, T, wave, lane);
  store_owned(reinterpret_cast<float*>(lds_raw), dv, 1.f, p.dv + at, pitch, kw, T, wave, lane);
}

}  // namespace

void launch_attention_forward(const AttnArgs& a, bool causal, hipStream_t stream) {
  if (a.D == 128) return launch_attention128_forward(a, causal, stream);
  with_instance(causal, [&](auto lv, auto cs) {
    hipLaunchKernelGGL((attention_fwd_kernel<decltype(lv)::value, decltype(cs)::value>),
                       attn_grid(a), dim3(kThreads), 0, stream, a);
  });
}

void launch_attention_backward(const AttnArgs& a, bool causal, hipStream_t stream) {
  if (a.D == 128) return launch_attention128_backward(a, causal, stream);
  hipLaunchKernelGGL(attention_delta_kernel, attn_grid(a), dim3(kThreads), 0, stream, a);
  with_instance(causal, [&](auto lv, auto cs) {
    hipLaunchKernelGGL((attention_dkv_kernel<decltype(lv)::value, decltype(cs)::value>),
                       attn_grid(a), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL((attention_dq_kernel<decltype(lv)::value, decltype(cs)::value>),
                       attn_grid(a), dim3(kThreads), 0, stream, a);
  });
}

}  // namespace tgpipe
