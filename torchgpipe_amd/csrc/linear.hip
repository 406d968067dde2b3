// Dense fp32 GEMMs of nn.Linear on the bf16 matrix pipes of gfx950 (split-bf16 products on
// v_mfma_f32_32x32x16_bf16, f32 accumulators): the arithmetic of conv_gemm.hip's EMU
// configurations (split1, the six partial products small parts first, the precision levels of
// conv_precision) on row-major matrices instead of NCHW planes.
//
// One core computes C[m][n] = sum_k A(m, k) B(n, k), C row-major [M][N], for the three
// passes of a Linear layer x[R][I], w[O][I], y[R][O]:
//
//   pass             C    M  N  K   A                          B
//   0 forward        y    R  O  I   x   [m][k]  k-contiguous   w [n][k]  k-contiguous
//   1 backward-data  dx   R  I  O   dy  [m][k]  k-contiguous   w [k][n]  k in rows
//   2 weight grad    dw   O  I  R   dy  [k][m]  k in rows      x [k][n]  k in rows
//
// Both orientations land in the same LDS image, the bf16 planes [k/8][row ^ 2(k/8)][8 k] the
// MFMA fragments read with one ds_read_b128 per lane half (emu_off), so there is one MFMA
// loop:
//   * k-contiguous (KC): a thread loads quads of four consecutive k of one row (16 bytes),
//     splits them and stores 8-byte bf16 quads;
//   * k in rows (KR): a thread loads four consecutive k rows of the same four columns, the
//     lanes of each load instruction along the contiguous columns (a wave reads two runs of
//     512 bytes), transposes the 4 x 4 block in registers and stores four k quads.  A KR
//     operand has 16 elements per unit, so half of the workgroup's waves stage it: the lower
//     half a KR A, the upper half a KR B (the weight gradient splits the waves evenly).
// An operand whose contiguous dimension is no multiple of 4, or whose base is not 16-byte
// aligned, is staged by the same units with one dword per load (a wave-uniform branch per
// operand, chosen on the host).
//
// Tails: rows, columns and k outside the matrices read 0 through raw buffer loads at an
// offset past the tensor (kOOB).  Row / column tails are folded into the per-thread base
// offsets once; the k tail can only be in a split's last stage, which is peeled off and
// alone computes its offsets with comparisons -- the main loop adds the stage's k offset to
// the bases and nothing else.
//
// Tiles: 128 x 128 (8 waves, 2 x 4 of 64 x 32) and 64 x 64 (4 waves, 2 x 2 of 32 x 32),
// BK = 32, two LDS buffers, one barrier per stage; the next stage's global loads are issued
// ahead of the stage's MFMAs and split / stored behind them.  grid.z splits the reduction
// when the tile grid leaves CUs idle: split z stores its partial tile into slice z of a
// workspace and linear_split_reduce_kernel sums the slices in order and applies the epilogue
// (bias / accumulate) -- no atomics, bitwise reproducible, nothing the host waits for.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "kernels.h"

namespace tgpipe {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 32;
constexpr uint32_t kOOB = 0x7ffffff0u;  // buffer offset past every tensor (< 2 GiB)
constexpr int kCUs = 256;               // MI355X

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const float* p, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), static_cast<short>(0),
                                           static_cast<int>(bytes), 0x00020000);
}

__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}

__device__ __forceinline__ floatx4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return floatx4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                 __uint_as_float(v[3])};
}

// conv_gemm.hip's image: slot j = k / 8 of row `row`, in bf16 elements
template <int ROWS>
__device__ __forceinline__ int emu_off(int j, int row) {
  return (j * ROWS + (row ^ (2 * j))) * 8;
}

// k quad q (k = 4q .. 4q+3) of `row` into the first 3 - LV planes (hi, mid, lo; the split
// of conv_gemm.hip's split1: round to nearest, each part of the remainder of the one before).
// A reduced level never forms the planes it does not multiply.
template <int ROWS, int LV>
__device__ __forceinline__ void store_quad(__bf16* img, const floatx4& v, int row, int q) {
  constexpr int kPlane = kBK * ROWS;
  bf16x4 hi, mid, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hi[e] = static_cast<__bf16>(v[e]);
    if constexpr (LV < 2) {
      const float r = v[e] - static_cast<float>(hi[e]);
      mid[e] = static_cast<__bf16>(r);
      if constexpr (LV == 0) lo[e] = static_cast<__bf16>(r - static_cast<float>(mid[e]));
    }
  }
  __bf16* p = img + emu_off<ROWS>(q >> 1, row) + 4 * (q & 1);
  *reinterpret_cast<bf16x4*>(p) = hi;
  if constexpr (LV < 2) *reinterpret_cast<bf16x4*>(p + kPlane) = mid;
  if constexpr (LV == 0) *reinterpret_cast<bf16x4*>(p + 2 * kPlane) = lo;
}

template <int TILE>
struct Tile {
  static_assert(TILE == 64 || TILE == 128, "64 x 64 or 128 x 128");
  static constexpr int WVM = 2, WVN = TILE == 128 ? 4 : 2;
  static constexpr int TM = TILE == 128 ? 2 : 1;  // 32 x 32 MFMA tiles per wave (rows)
  static constexpr int kThreads = 64 * WVM * WVN;
  // 128: one workgroup of 96 KiB per CU (two waves per SIMD); 64: three of 48 KiB
  static constexpr int kWavesPerSimd = TILE == 128 ? 2 : 3;
  static constexpr int kCStride = TILE + 8;  // rows 4 apart land 32 banks apart
  static constexpr int img(int lv) { return (3 - lv) * kBK * TILE; }  // bf16 per operand
  static constexpr int lds_bytes(int lv) {
    return 2 * 2 * img(lv) * 2 > TILE * kCStride * 4 ? 2 * 2 * img(lv) * 2
                                                    : TILE * kCStride * 4;
  }
};

// One operand's staging: the registers of a stage in flight and the per-thread base offsets.
// ROWS x BK elements per stage; T threads.  `row0` is the tile's first row (A: m0, B: n0),
// `rows` the operand's extent in that dimension, `ld` its leading dimension in elements.
template <int ROWS, int T, bool KR, int LV>
struct Stager {
  static constexpr int kRegs = KR ? 4 : 2;
  floatx4 v[kRegs];
  uint32_t base[kRegs];  // KC: per unit (row); KR: per column of the 4 x 4 block
  int q;                 // k quad of the unit(s)
  int r;                 // KC: row of unit 0 (unit 1: + T / 8); KR: first of the 4 rows
  uint32_t ldb;          // KR: bytes between k rows
  bool vec, active;

  // `u`: the thread's index among the threads staging this operand
  __device__ __forceinline__ void init(int u, bool on, int row0, int rows, int ld, bool vec_) {
    vec = vec_;
    active = on;
    ldb = static_cast<uint32_t>(ld) * 4u;
    if constexpr (KR) {
      q = u / (ROWS / 4);
      r = 4 * (u % (ROWS / 4));
#pragma unroll
      for (int c = 0; c < 4; ++c)
        base[c] = row0 + r + c < rows ? static_cast<uint32_t>(row0 + r + c) * 4u : kOOB;
    } else {
      q = u & 7;
      r = u >> 3;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rg = row0 + r + (T / 8) * i;
        base[i] = rg < rows ? (static_cast<uint32_t>(rg) * static_cast<uint32_t>(ld) + 4u * q) * 4u
                            : kOOB;
      }
    }
  }

  // the stage of k0 .. k0+31; TAIL: k >= k_end reads 0 (a base at kOOB stays past the
  // tensor whatever k offset is added: the sum is below 2^32)
  template <bool TAIL>
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, int k0, int k_end) {
    if (!active) return;
    if constexpr (KR) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 4 * q + e;
        const uint32_t koff = static_cast<uint32_t>(k) * ldb;
        const bool in = !TAIL || k < k_end;
        if (vec) {
          v[e] = bload4(rs, in ? base[0] + koff : kOOB);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) v[e][c] = bload(rs, in ? base[c] + koff : kOOB);
        }
      }
    } else {
      const uint32_t koff = static_cast<uint32_t>(k0) * 4u;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (vec) {  // (k0 + 4q and k_end are multiples of 4 here: the quad is in or out)
          v[i] = bload4(rs, !TAIL || k0 + 4 * q < k_end ? base[i] + koff : kOOB);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[i][e] = bload(rs, !TAIL || k0 + 4 * q + e < k_end ? base[i] + koff + 4u * e : kOOB);
        }
      }
    }
  }

  __device__ __forceinline__ void store(__bf16* img) const {
    if (!active) return;
    if constexpr (KR) {
#pragma unroll
      for (int c = 0; c < 4; ++c)  // the 4 x 4 transpose: column c of the block is a k quad
        store_quad<ROWS, LV>(img, floatx4{v[0][c], v[1][c], v[2][c], v[3][c]}, r + c, q);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) store_quad<ROWS, LV>(img, v[i], r + (T / 8) * i, q);
    }
  }
};

struct LinearArgs {
  const float* a;
  const float* b;
  const float* bias;  // [N] added to every row, or null
  float* out;         // C, or the split workspace
  int M, N, K, k_chunk;
  int lda, ldb;
  int64_t split_stride;  // floats between the workspace slices of two splits
  int64_t a_bytes, b_bytes;
  int a_vec, b_vec, c_vec;
  int accumulate;  // C += (not with splits: the reduction accumulates)
};

// Two k steps of 16; per 32 x 32 tile and step the level's partial products, small parts
// first (conv_gemm.hip kPairs).  Fragments are read per step.
template <int TILE, int LV>
__device__ __forceinline__ void mfma_stage(floatx16 (&acc)[Tile<TILE>::TM], const __bf16* ab,
                                           const __bf16* bb, int lane, int wm, int wn) {
  constexpr int TM = Tile<TILE>::TM, P = 3 - LV, kPlane = kBK * TILE;
  constexpr int kPairs[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};
  constexpr int T0 = LV == 0 ? 0 : (LV == 1 ? 3 : 5);
  const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
  for (int s = 0; s < kBK / 16; ++s) {
    bf16x8 a[P][TM], b[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[p][i] = *reinterpret_cast<const bf16x8*>(
            ab + p * kPlane + emu_off<TILE>(2 * s + h, wm * 32 * TM + i * 32 + l32));
      b[p] = *reinterpret_cast<const bf16x8*>(
          bb + p * kPlane + emu_off<TILE>(2 * s + h, wn * 32 + l32));
    }
#pragma unroll
    for (int t = T0; t < 6; ++t)
#pragma unroll
      for (int i = 0; i < TM; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kPairs[t][0]][i], b[kPairs[t][1]],
                                                         acc[i], 0, 0, 0);
  }
}

template <int TILE, bool AKR, bool BKR, int LV>
__global__ __launch_bounds__(Tile<TILE>::kThreads, Tile<TILE>::kWavesPerSimd) void
linear_gemm_kernel(LinearArgs p) {
  using C = Tile<TILE>;
  constexpr int T = C::kThreads, TM = C::TM, kImg = C::img(LV);
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[C::lds_bytes(LV)];
  __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / C::WVN, wn = wave % C::WVN;
  const int mb = (p.M + TILE - 1) / TILE;
  // row blocks fastest: neighbouring workgroups share B's column block (the weight in the
  // forward and backward-data passes) while it is in cache
  const int m0 = (blockIdx.x % mb) * TILE, n0 = (blockIdx.x / mb) * TILE;
  const int k_begin = blockIdx.z * p.k_chunk;
  const int k_end = min(p.K, k_begin + p.k_chunk);

  const __amdgpu_buffer_rsrc_t ar = rsrc(p.a, p.a_bytes), br = rsrc(p.b, p.b_bytes);
  Stager<TILE, T, AKR, LV> sa;
  Stager<TILE, T, BKR, LV> sb;
  // a KR operand is staged by half of the threads: A by the lower, B by the upper half
  sa.init(tid, !AKR || tid < T / 2, m0, p.M, p.lda, p.a_vec != 0);
  sb.init(BKR ? (tid + T / 2) % T : tid, !BKR || tid >= T / 2, n0, p.N, p.ldb, p.b_vec != 0);

  floatx16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  auto aimg = [&](int buf) { return lds + buf * 2 * kImg; };
  auto bimg = [&](int buf) { return lds + buf * 2 * kImg + kImg; };

  const int stages = (k_end - k_begin + kBK - 1) / kBK;
  if (stages > 0) {
    sa.template load<true>(ar, k_begin, k_end);
    sb.template load<true>(br, k_begin, k_end);
    sa.store(aimg(0));
    sb.store(bimg(0));
    __syncthreads();
    auto step = [&](int s, auto tail_c) {
      constexpr bool kTail = decltype(tail_c)::value;
      const int buf = s & 1, k_next = k_begin + (s + 1) * kBK;
      sa.template load<kTail>(ar, k_next, k_end);
      sb.template load<kTail>(br, k_next, k_end);
      mfma_stage<TILE, LV>(acc, aimg(buf), bimg(buf), lane, wm, wn);
      sa.store(aimg(buf ^ 1));
      sb.store(bimg(buf ^ 1));
      __syncthreads();
    };
    int s = 0;
    for (; s + 2 < stages; ++s) step(s, std::false_type{});
    if (stages >= 2) step(s, std::true_type{});  // loads the split's last stage: the k tail
    mfma_stage<TILE, LV>(acc, aimg((stages - 1) & 1), bimg((stages - 1) & 1), lane, wm, wn);
    __syncthreads();
  }

  // ---- epilogue: the C tile through LDS (over the operand images), coalesced row stores ----
  float* ct = reinterpret_cast<float*>(lds_raw);
  {
    const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        ct[row * C::kCStride + wn * 32 + l32] = acc[i][r];
      }
  }
  __syncthreads();

  float* out = p.out + blockIdx.z * p.split_stride;
  constexpr int kQuads = TILE / 4;
  for (int idx = tid; idx < TILE * kQuads; idx += T) {
    const int row = idx / kQuads, q = idx - row * kQuads;
    const int m = m0 + row, n = n0 + 4 * q;
    if (m >= p.M || n >= p.N) continue;
    floatx4 v = *reinterpret_cast<const floatx4*>(ct + row * C::kCStride + 4 * q);
    float* o = out + static_cast<int64_t>(m) * p.N + n;
    if (p.c_vec) {  // N is a multiple of 4: the quad is inside the row
      if (p.bias) v += *reinterpret_cast<const floatx4*>(p.bias + n);
      if (p.accumulate) v += *reinterpret_cast<const floatx4*>(o);
      *reinterpret_cast<floatx4*>(o) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n + e >= p.N) break;
        float val = v[e];
        if (p.bias) val += p.bias[n + e];
        if (p.accumulate) val += o[e];
        o[e] = val;
      }
    }
  }
}

// out[m][n] (+)= sum_s ws[s][m][n] (+ bias[n]), the slices in order.  VEC: four elements per
// thread (N a multiple of 4, 16-byte aligned pointers).
template <bool VEC>
__global__ __launch_bounds__(256) void linear_split_reduce_kernel(
    const float* __restrict__ ws, int splits, int64_t stride, const float* __restrict__ bias,
    float* out, int N, int64_t total, int accumulate) {
  constexpr int E = VEC ? 4 : 1;
  const int64_t idx = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * E;
  if (idx >= total) return;
  if constexpr (VEC) {
    floatx4 v = *reinterpret_cast<const floatx4*>(ws + idx);
    for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const floatx4*>(ws + s * stride + idx);
    if (bias) v += *reinterpret_cast<const floatx4*>(bias + idx % N);
    if (accumulate) v += *reinterpret_cast<const floatx4*>(out + idx);
    *reinterpret_cast<floatx4*>(out + idx) = v;
  } else {
    float v = ws[idx];
    for (int s = 1; s < splits; ++s) v += ws[s * stride + idx];
    if (bias) v += bias[idx % N];
    if (accumulate) v += out[idx];
    out[idx] = v;
  }
}

// db[o] (+)= sum_r dy[r][o]: 32 columns per workgroup, eight row groups of 32 lanes (128
// contiguous bytes per group and row); a group sums its rows r = g, g + 8, ... in order,
// then the eight partial sums are added in order.
__global__ __launch_bounds__(256) void linear_bias_grad_kernel(const float* __restrict__ dy,
                                                               float* db, int R, int O,
                                                               int accumulate) {
  __shared__ float part[8][32];
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int o = blockIdx.x * 32 + c;
  float s = 0.f;
  if (o < O)
    for (int r = g; r < R; r += 8) s += dy[static_cast<int64_t>(r) * O + o];
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && o < O) {
    float t = part[0][c];
#pragma unroll
    for (int i = 1; i < 8; ++i) t += part[i][c];
    db[o] = accumulate ? db[o] + t : t;
  }
}

std::atomic<int> forced_tile{-1};
std::atomic<int> forced_splits{-1};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int TILE, bool AKR, bool BKR>
void launch_tile(const LinearArgs& args, int splits, hipStream_t stream) {
  const int mb = (args.M + TILE - 1) / TILE, nb = (args.N + TILE - 1) / TILE;
  const dim3 grid(mb * nb, 1, splits), block(Tile<TILE>::kThreads);
  // the level in force picks the instance (read at launch: a captured graph keeps its own)
  switch (conv_precision_level()) {
    case 1:
      hipLaunchKernelGGL((linear_gemm_kernel<TILE, AKR, BKR, 1>), grid, block, 0, stream, args);
      break;
    case 2:
      hipLaunchKernelGGL((linear_gemm_kernel<TILE, AKR, BKR, 2>), grid, block, 0, stream, args);
      break;
    default:
      hipLaunchKernelGGL((linear_gemm_kernel<TILE, AKR, BKR, 0>), grid, block, 0, stream, args);
  }
}

}  // namespace

void linear_force_plan(int tile, int splits) {
  forced_tile.store(tile == 64 || tile == 128 ? tile : -1);
  forced_splits.store(splits >= 1 ? splits : -1);
}

// The host rule.  Tile: 128 x 128 when both extents pass 64 (half the operand traffic per
// product of the 64 x 64 tile), else 64 x 64 (a 64-row micro-batch wastes no MFMA rows).
// Splits: when the tiles do not fill the CUs (twice over for the small tile, whose
// workgroups share a CU), split the reduction, no finer than 256 deep and at most 16 ways.
LinearPlan linear_plan(int M, int N, int K) {
  LinearPlan plan;
  const int ft = forced_tile.load(), fs = forced_splits.load();
  plan.tile = ft > 0 ? ft : (M > 64 && N > 64 ? 128 : 64);
  const int64_t tiles = static_cast<int64_t>((M + plan.tile - 1) / plan.tile) *
                        ((N + plan.tile - 1) / plan.tile);
  int splits = 1;
  if (fs > 0) {
    splits = fs;
  } else {
    const int64_t target = plan.tile == 128 ? kCUs : 2 * kCUs;
    splits = static_cast<int>(std::min<int64_t>({target / tiles, K / 256, 16}));
  }
  splits = std::max(1, splits);
  int k_chunk = (K + splits - 1) / splits;
  k_chunk = (k_chunk + kBK - 1) / kBK * kBK;  // whole BK stages per split
  plan.k_chunk = k_chunk;
  plan.splits = (K + k_chunk - 1) / k_chunk;
  return plan;
}

int64_t linear_workspace(int M, int N, const LinearPlan& plan) {
  return plan.splits > 1 ? static_cast<int64_t>(plan.splits) * M * N : 0;
}

void launch_linear_gemm(int pass, const float* a, const float* b, const float* bias, float* out,
                        int M, int N, int K, const LinearPlan& plan, bool accumulate, float* ws,
                        hipStream_t stream) {
  const bool split = plan.splits > 1;
  LinearArgs args;
  args.a = a;
  args.b = b;
  args.bias = split ? nullptr : bias;
  args.out = split ? ws : out;
  args.M = M;
  args.N = N;
  args.K = K;
  args.k_chunk = plan.k_chunk;
  args.lda = pass == 2 ? M : K;
  args.ldb = pass == 0 ? K : N;
  args.split_stride = split ? static_cast<int64_t>(M) * N : 0;
  args.a_bytes = static_cast<int64_t>(M) * K * 4;
  args.b_bytes = static_cast<int64_t>(N) * K * 4;
  args.a_vec = args.lda % 4 == 0 && aligned16(a);
  args.b_vec = args.ldb % 4 == 0 && aligned16(b);
  args.c_vec = N % 4 == 0 && aligned16(args.out) && (!args.bias || aligned16(args.bias));
  args.accumulate = !split && accumulate;
  auto go = [&](auto tile_c) {
    constexpr int TILE = decltype(tile_c)::value;
    if (pass == 0) launch_tile<TILE, false, false>(args, plan.splits, stream);
    else if (pass == 1) launch_tile<TILE, false, true>(args, plan.splits, stream);
    else launch_tile<TILE, true, true>(args, plan.splits, stream);
  };
  if (plan.tile == 128) go(std::integral_constant<int, 128>{});
  else go(std::integral_constant<int, 64>{});
  if (!split) return;
  const int64_t total = static_cast<int64_t>(M) * N;
  const bool vec = N % 4 == 0 && aligned16(ws) && aligned16(out) && (!bias || aligned16(bias));
  const int64_t threads = vec ? total / 4 : total;
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256));
  if (vec)
    hipLaunchKernelGGL(linear_split_reduce_kernel<true>, grid, dim3(256), 0, stream, ws,
                       plan.splits, total, bias, out, N, total, accumulate ? 1 : 0);
  else
    hipLaunchKernelGGL(linear_split_reduce_kernel<false>, grid, dim3(256), 0, stream, ws,
                       plan.splits, total, bias, out, N, total, accumulate ? 1 : 0);
}

void launch_linear_bias_grad(const float* dy, float* db, int R, int O, bool accumulate,
                             hipStream_t stream) {
  hipLaunchKernelGGL(linear_bias_grad_kernel, dim3((O + 31) / 32), dim3(256), 0, stream, dy, db,
                     R, O, accumulate ? 1 : 0);
}

}  // namespace tgpipe
