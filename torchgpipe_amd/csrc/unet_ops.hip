// U-Net's resolution changes as single passes (models/unet.py):
//
//   up2x_cat:    cat(nearest_upsample_2x(x), skip) along channels -- the decoder's 'up' +
//                'skip' layers (reference: nn.Upsample(scale_factor=2) then torch.cat); one
//                read of x and skip, one write of the concatenation, instead of writing the
//                upsampled tensor and copying it again.
//   up2x_bwd:    dx[n][c][y][x] = sum of the 2x2 block of dy's first C channels; dy may be
//                the channel slice of the concatenation's gradient (read in place).
//   maxpool2x2:  nn.MaxPool2d(2, stride=2) without the int64 index tensor (ATen writes one
//                per output: 3x the output traffic); the backward re-finds the argmax from
//                the input, which the U-Net keeps alive anyway (it is the stashed skip).
//                Ties and NaN follow ATen: the first maximum in row-major window order wins,
//                NaN wins over numbers (the last NaN of a window).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tgpipe {
namespace {

typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// Element types: float, and __bf16 as storage -- sums and `m + add` are computed in f32 and
// stored rounded to nearest even, once; comparisons on the upcast value are exact.
template <typename E>
struct Pair;
template <>
struct Pair<float> {
  typedef floatx2 type;
};
template <>
struct Pair<__bf16> {
  typedef bf16x2 type;
};

unsigned grid_for(int64_t work) {
  const int64_t b = (work + 255) / 256;
  return static_cast<unsigned>(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

// One thread per pair of output columns (W even: the pair shares one upsampled source).
template <typename E>
__global__ __launch_bounds__(256) void up2x_cat_kernel(const E* __restrict__ x,
                                                       const E* __restrict__ skip,
                                                       E* __restrict__ out, int64_t n,
                                                       int c1, int c2, int h, int w) {
  typedef typename Pair<E>::type P;
  const int H = 2 * h, W = 2 * w, ct = c1 + c2;
  const int64_t pairs = n * ct * H * w;  // output element pairs
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < pairs;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t plane = i / (static_cast<int64_t>(H) * w);
    const int r = static_cast<int>(i - plane * H * w);
    const int oy = r / w, ox2 = r - oy * w;  // output row, column pair
    const int64_t img = plane / ct;
    const int ch = static_cast<int>(plane - img * ct);
    P v;
    if (ch < c1) {
      const E s = x[((img * c1 + ch) * h + (oy >> 1)) * w + ox2];
      v = P{s, s};
    } else {
      v = *reinterpret_cast<const P*>(
          skip + ((img * c2 + (ch - c1)) * H + oy) * static_cast<int64_t>(W) + 2 * ox2);
    }
    *reinterpret_cast<P*>(out + (plane * H + oy) * static_cast<int64_t>(W) + 2 * ox2) = v;
  }
}

template <typename E>
__global__ __launch_bounds__(256) void up2x_bwd_kernel(const E* __restrict__ dy,
                                                       E* __restrict__ dx, int64_t n, int c,
                                                       int h, int w, int64_t dy_img) {
  typedef typename Pair<E>::type P;
  const int W = 2 * w;
  const int64_t total = n * c * h * w;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t plane = i / (static_cast<int64_t>(h) * w);
    const int r = static_cast<int>(i - plane * h * w);
    const int y = r / w, xx = r - y * w;
    const int64_t img = plane / c;
    const E* g = dy + img * dy_img + ((plane - img * c) * 2 * h + 2 * y) * W + 2 * xx;
    const P a = *reinterpret_cast<const P*>(g);
    const P b = *reinterpret_cast<const P*>(g + W);
    dx[i] = static_cast<E>((static_cast<float>(a[0]) + static_cast<float>(a[1])) +
                           (static_cast<float>(b[0]) + static_cast<float>(b[1])));
  }
}

// ATen's scan: start from -inf, a later element replaces the maximum when it is strictly
// larger or NaN (so the first of equal maxima and the last NaN win).
__device__ __forceinline__ int argmax4(float v0, float v1, float v2, float v3, float& m) {
  const float v[4] = {v0, v1, v2, v3};
  int k = 0;
  m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (v[j] > m || isnan(v[j])) {
      m = v[j];
      k = j;
    }
  }
  return k;
}

template <typename E>
__global__ __launch_bounds__(256) void maxpool2x2_fwd_kernel(const E* __restrict__ x,
                                                             const E* __restrict__ add,
                                                             E* __restrict__ y,
                                                             int64_t planes, int h, int w) {
  const int ho = h / 2, wo = w / 2;
  const int64_t total = planes * ho * wo;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t plane = i / (static_cast<int64_t>(ho) * wo);
    const int r = static_cast<int>(i - plane * ho * wo);
    const int oy = r / wo, ox = r - oy * wo;
    const E* p = x + (plane * h + 2 * oy) * static_cast<int64_t>(w) + 2 * ox;
    float m;
    argmax4(static_cast<float>(p[0]), static_cast<float>(p[1]), static_cast<float>(p[w]),
            static_cast<float>(p[w + 1]), m);
    // AmoebaNet's cell-node sum folded in
    y[i] = static_cast<E>(add != nullptr ? m + static_cast<float>(add[i]) : m);
  }
}

// One thread per 2x2 input block: writes all four input gradients (zeros but the argmax),
// so every input element is written exactly once (odd trailing rows / columns, which no
// window covers, are zeroed by the caller's allocation).  dy may be a channel slice of a
// larger gradient (image stride dy_img, e.g. AmoebaNet's concatenated cell output).
template <typename E>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const E* __restrict__ x,
                                                             const E* __restrict__ dy,
                                                             E* __restrict__ dx,
                                                             int64_t planes, int channels,
                                                             int h, int w, int64_t dy_img) {
  const int ho = h / 2, wo = w / 2;
  const int64_t total = planes * ho * wo;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t plane = i / (static_cast<int64_t>(ho) * wo);
    const int r = static_cast<int>(i - plane * ho * wo);
    const int oy = r / wo, ox = r - oy * wo;
    const int64_t base = (plane * h + 2 * oy) * static_cast<int64_t>(w) + 2 * ox;
    const E* p = x + base;
    float m;
    const int k = argmax4(static_cast<float>(p[0]), static_cast<float>(p[1]),
                          static_cast<float>(p[w]), static_cast<float>(p[w + 1]), m);
    const int64_t img = plane / channels;
    const E g = dy[img * dy_img + (plane - img * channels) * ho * wo + r];
    const E zero = static_cast<E>(0.f);
    E* q = dx + base;
    q[0] = k == 0 ? g : zero;
    q[1] = k == 1 ? g : zero;
    q[w] = k == 2 ? g : zero;
    q[w + 1] = k == 3 ? g : zero;
  }
}

typedef float floatx4 __attribute__((ext_vector_type(4)));

// ResNet's residual join: y = relu(x + identity), one pass (the sum and the ReLU were two
// ATen passes over the block output).  A NaN sum stays NaN, as in ATen's relu (and in the
// max pool above): a diverged branch must show at the join, not vanish into a 0.
__device__ __forceinline__ float relu_nan(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }

__global__ __launch_bounds__(256) void add_relu_kernel(const float* __restrict__ a,
                                                       const float* __restrict__ b,
                                                       float* __restrict__ y, int64_t quads,
                                                       int64_t total) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; q < quads; q += stride) {
    const floatx4 v =
        reinterpret_cast<const floatx4*>(a)[q] + reinterpret_cast<const floatx4*>(b)[q];
    floatx4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = relu_nan(v[e]);
    reinterpret_cast<floatx4*>(y)[q] = o;
  }
  // tail (total % 4), by the first workgroup
  if (blockIdx.x == 0) {
    const int64_t i = quads * 4 + threadIdx.x;
    if (i < total) {
      y[i] = relu_nan(a[i] + b[i]);
    }
  }
}

}  // namespace

void launch_add_relu(const float* a, const float* b, float* y, int64_t total,
                     hipStream_t stream) {
  if (total == 0) return;
  const int64_t quads = total / 4;
  int64_t blocks = (quads + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
  hipLaunchKernelGGL(add_relu_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream,
                     a, b, y, quads, total);
}

namespace {

template <typename E>
void up2x_cat_any(const E* x, const E* skip, E* out, int64_t n, int c1, int c2, int h, int w,
                  hipStream_t stream) {
  const int64_t pairs = n * (c1 + c2) * 2 * static_cast<int64_t>(h) * w;
  if (pairs == 0) return;
  hipLaunchKernelGGL(up2x_cat_kernel<E>, dim3(grid_for(pairs)), dim3(256), 0, stream, x, skip,
                     out, n, c1, c2, h, w);
}

template <typename E>
void up2x_backward_any(const E* dy, E* dx, int64_t n, int c, int h, int w, int64_t dy_img,
                       hipStream_t stream) {
  const int64_t total = n * c * static_cast<int64_t>(h) * w;
  if (total == 0) return;
  hipLaunchKernelGGL(up2x_bwd_kernel<E>, dim3(grid_for(total)), dim3(256), 0, stream, dy, dx, n,
                     c, h, w, dy_img);
}

template <typename E>
void maxpool2x2_forward_any(const E* x, const E* add, E* y, int64_t planes, int h, int w,
                            hipStream_t stream) {
  const int64_t total = planes * (h / 2) * static_cast<int64_t>(w / 2);
  if (total == 0) return;
  hipLaunchKernelGGL(maxpool2x2_fwd_kernel<E>, dim3(grid_for(total)), dim3(256), 0, stream, x,
                     add, y, planes, h, w);
}

template <typename E>
void maxpool2x2_backward_any(const E* x, const E* dy, E* dx, int64_t planes, int channels, int h,
                             int w, int64_t dy_img, hipStream_t stream) {
  const int64_t total = planes * (h / 2) * static_cast<int64_t>(w / 2);
  if (total == 0) return;
  hipLaunchKernelGGL(maxpool2x2_bwd_kernel<E>, dim3(grid_for(total)), dim3(256), 0, stream, x,
                     dy, dx, planes, channels, h, w, dy_img);
}

const __bf16* bf(const bf16_bits* p) { return reinterpret_cast<const __bf16*>(p); }
__bf16* bf(bf16_bits* p) { return reinterpret_cast<__bf16*>(p); }

}  // namespace

void launch_up2x_cat(const float* x, const float* skip, float* out, int64_t n, int c1, int c2,
                     int h, int w, hipStream_t stream) {
  up2x_cat_any(x, skip, out, n, c1, c2, h, w, stream);
}
void launch_up2x_cat(const bf16_bits* x, const bf16_bits* skip, bf16_bits* out, int64_t n,
                     int c1, int c2, int h, int w, hipStream_t stream) {
  up2x_cat_any(bf(x), bf(skip), bf(out), n, c1, c2, h, w, stream);
}

void launch_up2x_backward(const float* dy, float* dx, int64_t n, int c, int h, int w,
                          int64_t dy_img, hipStream_t stream) {
  up2x_backward_any(dy, dx, n, c, h, w, dy_img, stream);
}
void launch_up2x_backward(const bf16_bits* dy, bf16_bits* dx, int64_t n, int c, int h, int w,
                          int64_t dy_img, hipStream_t stream) {
  up2x_backward_any(bf(dy), bf(dx), n, c, h, w, dy_img, stream);
}

void launch_maxpool2x2_forward(const float* x, const float* add, float* y, int64_t planes, int h,
                               int w, hipStream_t stream) {
  maxpool2x2_forward_any(x, add, y, planes, h, w, stream);
}
void launch_maxpool2x2_forward(const bf16_bits* x, const bf16_bits* add, bf16_bits* y,
                               int64_t planes, int h, int w, hipStream_t stream) {
  maxpool2x2_forward_any(bf(x), bf(add), bf(y), planes, h, w, stream);
}

void launch_maxpool2x2_backward(const float* x, const float* dy, float* dx, int64_t planes,
                                int channels, int h, int w, int64_t dy_img, hipStream_t stream) {
  maxpool2x2_backward_any(x, dy, dx, planes, channels, h, w, dy_img, stream);
}
void launch_maxpool2x2_backward(const bf16_bits* x, const bf16_bits* dy, bf16_bits* dx,
                                int64_t planes, int channels, int h, int w, int64_t dy_img,
                                hipStream_t stream) {
  maxpool2x2_backward_any(bf(x), bf(dy), bf(dx), planes, channels, h, w, dy_img, stream);
}

}  // namespace tgpipe
