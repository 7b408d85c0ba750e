// The dense categorical image path (image_encoder = image_decoder = 'dense', image_categorical: the `minigrid` section of
// defaults.yaml): what DenseEncoder (encoders.py:99-125) and CatImageDecoder (decoders.py:183-254) need beyond the MLP of
// mlp.hip and the per-cell kernels of cat_image.hip.
//   * dm_dense_image_rows: the encoder's input rows - the categorical image with the reward / terminal planes of reward_input
//     behind it (encoders.py:50-61), flattened class-major as nn.Flatten lays a (C+2, H, W) block out;
//   * dm_elu_rows_fwd / _bwd: the activation() behind DenseEncoder's last Linear (encoders.py:116-118; the library's MLP ends
//     in a bare Linear), on the element-wise ELU kernels of elementwise.hip;
//   * dm_cat_image_loss_mix: CatImageDecoder.loss with min_prob > 0 (decoders.py:229-231), the softmax mixed with the uniform
//     distribution before the logarithm.  Lanes over cells, classes inside a lane, the row sum through a shuffle tree and LDS in
//     a fixed order - the layout of cat_image_loss_kernel, no float atomics.
// Everything is fp32; the paths are small (1 536 rows of 294 inputs / 196 logits at the minigrid batch).
#include "common.h"

#include <math.h>

namespace {

constexpr int DI_THREADS = 256;
constexpr int DI_WAVES = DI_THREADS / 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;      // complete in lane 0
}

// out[r][j], j < W = (C + 2 * planes) * cells: class c = j / cells of cell p = j % cells for c < C, then the reward plane, then the
// terminal plane.  A float source is copied as it is; a class source is compared (a class outside [0, C) matches no c).
__global__ void __launch_bounds__(DI_THREADS) dense_image_rows_kernel(long long total, int C, int cells, int W,
                                                                      const float* __restrict__ image, const int* __restrict__ cls,
                                                                      const float* __restrict__ reward,
                                                                      const float* __restrict__ terminal, float* __restrict__ out,
                                                                      int ldo) {
  const int n = C * cells;
  for (long long e = (long long)blockIdx.x * DI_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * DI_THREADS) {
    const long long r = e / W;
    const int j = (int)(e - r * W);
    float v;
    if (j < n) {
      if (image) {
        v = image[(size_t)r * n + j];
      } else {
        const int c = j / cells;
        v = cls[(size_t)r * cells + (j - c * cells)] == c ? 1.f : 0.f;
      }
    } else {
      v = j < n + cells ? reward[r] : terminal[r];
    }
    out[(size_t)r * ldo + j] = v;
  }
}

// One row per group of `wpr` waves, as cat_image_loss_kernel.  Per cell: s = softmax_c x, p_t = (1 - m) s_t + m / C,
// loss += -log p_t, dlogits_c = -(1 - m) s_t (delta_ct - s_c) / p_t.  s_t is picked up inside the class loop: a target outside
// [0, C) reads nothing out of bounds (s_t = 0: the cell contributes -log(m / C) and a zero gradient).  p_t >= m / C > 0, so the
// logarithm and the quotient stay finite when s_t underflows.
__global__ void __launch_bounds__(DI_THREADS) cat_image_loss_mix_kernel(int rows, int I, int C, int cells, int wpr,
                                                                        const float* __restrict__ logits, int ld,
                                                                        const int* __restrict__ target, float keep, float floor_p,
                                                                        float* __restrict__ loss, float* __restrict__ dlogits) {
  __shared__ float part[DI_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rpb = DI_WAVES / wpr;
  const long long r = (long long)blockIdx.x * rpb + wave / wpr;
  const int sub = wave % wpr;
  float s = 0.f;
  if (r < rows) {
    const float* x = logits + (size_t)r * ld;
    const int* tg = target + (size_t)(r / I) * cells;
    float* d = dlogits ? dlogits + (size_t)r * C * cells : nullptr;
    for (int p = sub * 64 + lane; p < cells; p += wpr * 64) {
      const int t = tg[p];
      float m = x[p];
      for (int c = 1; c < C; ++c) m = fmaxf(m, x[(size_t)c * cells + p]);
      float z = 0.f, et = 0.f;
      for (int c = 0; c < C; ++c) {
        const float e = expf(x[(size_t)c * cells + p] - m);
        z += e;
        if (c == t) et = e;
      }
      const float rz = 1.f / z;
      const float st = et * rz;
      const float pt = keep * st + floor_p;
      s -= logf(pt);
      if (d) {
        const float g = keep * st / pt;      // -d loss / d s_t * s_t
        for (int c = 0; c < C; ++c)
          d[(size_t)c * cells + p] = g * (expf(x[(size_t)c * cells + p] - m) * rz - (c == t ? 1.f : 0.f));
      }
    }
  }
  s = wave_sum(s);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  if (r < rows && sub == 0 && lane == 0) {
    float acc = part[wave];
    for (int w = 1; w < wpr; ++w) acc += part[wave + w];
    loss[r] = acc;
  }
}

int ew_grid(long long total) {
  long long b = (total + DI_THREADS - 1) / DI_THREADS;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" int dm_dense_image_rows(int rows, int C, int cells, const float* image_f32, const int32_t* class_i32, const float* reward,
                                   const float* terminal, float* out, int ldo, void* stream) {
  DM_REQUIRE(out && ((image_f32 != nullptr) != (class_i32 != nullptr)), DM_E_NULL,
             "dense_image_rows: out and exactly one of image_f32 / class_i32 must be given");
  DM_REQUIRE((reward != nullptr) == (terminal != nullptr), DM_E_NULL, "dense_image_rows: reward and terminal come together");
  DM_REQUIRE(rows >= 0 && C >= 1 && cells >= 1, DM_E_SHAPE, "dense_image_rows: rows=%d C=%d cells=%d", rows, C, cells);
  const long long W = ((long long)C + (reward ? 2 : 0)) * cells;
  DM_REQUIRE(W <= 0x7fffffffLL && (long long)ldo >= W, DM_E_SHAPE, "dense_image_rows: ldo=%d < row width %lld", ldo, W);
  if (rows == 0) return DM_OK;
  const long long total = (long long)rows * W;
  hipLaunchKernelGGL(dense_image_rows_kernel, dim3(ew_grid(total)), dim3(DI_THREADS), 0, (hipStream_t)stream, total, C, cells, (int)W,
                     image_f32, class_i32, reward, terminal, out, ldo);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_elu_rows_fwd(int rows, int n, const float* x, int ldx, float* y, int ldy, void* stream) {
  DM_REQUIRE(x && y, DM_E_NULL, "elu_rows_fwd: null pointer");
  DM_REQUIRE(rows >= 0 && n >= 1 && ldx >= n && ldy >= n, DM_E_SHAPE, "elu_rows_fwd: rows=%d n=%d ldx=%d ldy=%d", rows, n, ldx, ldy);
  return dm_elu_fwd_launch(rows, n, x, ldx, y, ldy, (hipStream_t)stream);
}

extern "C" int dm_elu_rows_bwd(int rows, int n, const float* y, int ldy, const float* dy, int lddy, float* dx, int lddx,
                               void* stream) {
  DM_REQUIRE(y && dy && dx, DM_E_NULL, "elu_rows_bwd: null pointer");
  DM_REQUIRE(rows >= 0 && n >= 1 && ldy >= n && lddy >= n && lddx >= n, DM_E_SHAPE, "elu_rows_bwd: rows=%d n=%d ldy=%d lddy=%d lddx=%d",
             rows, n, ldy, lddy, lddx);
  return dm_elu_bwd_launch(rows, n, y, ldy, dy, lddy, dx, lddx, (hipStream_t)stream);
}

extern "C" int dm_cat_image_loss_mix(int rows, int I, int C, int cells, const float* logits, int ld, const int32_t* target,
                                     float min_prob, float* loss, float* dlogits, void* stream) {
  DM_REQUIRE(logits && target && loss, DM_E_NULL, "cat_image_loss_mix: null pointer");      // dlogits may be NULL (no backward)
  DM_REQUIRE(rows >= 0 && C >= 1 && cells >= 1 && I >= 1, DM_E_SHAPE, "cat_image_loss_mix: rows=%d C=%d cells=%d I=%d", rows, C, cells, I);
  DM_REQUIRE(rows % I == 0, DM_E_SHAPE, "cat_image_loss_mix: rows=%d is no multiple of I=%d", rows, I);
  DM_REQUIRE((long long)ld >= (long long)C * cells, DM_E_SHAPE, "cat_image_loss_mix: ld=%d < C*cells=%lld", ld, (long long)C * cells);
  DM_REQUIRE(min_prob > 0.f && min_prob < 1.f, DM_E_SHAPE, "cat_image_loss_mix: min_prob=%g outside (0, 1) (0: dm_cat_image_loss)",
             (double)min_prob);
  if (rows == 0) return DM_OK;
  const int wpr = cells <= 64 ? 1 : (cells <= 128 ? 2 : DI_WAVES);      // waves per row
  const int rpb = DI_WAVES / wpr;
  hipLaunchKernelGGL(cat_image_loss_mix_kernel, dim3(dm_cdiv(rows, rpb)), dim3(DI_THREADS), 0, (hipStream_t)stream, rows, I, C, cells,
                     wpr, logits, ld, target, 1.f - min_prob, min_prob / (float)C, loss, dlogits);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
