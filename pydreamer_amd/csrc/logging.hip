// The trainer loop's device-side logging (train.py:204-214, 346, 365-372, 452): four small kernels, each ONE launch - of ONE
// workgroup for the three reductions, of a grid for the elementwise image export.  The reductions' data is a few thousand values at
// most and the cost is launch latency, so the kernels are plain: no float atomics, no flags, no spin loops; the same inputs give the
// same bits.  Every reduction accumulates in fp64 in a fixed order - a thread's strided elements in sequence, then a fixed LDS tree
// over the 256 threads - and is rounded to fp32 once.
//   metric_accum_kernel     one thread per slot: folds a step's metric buffer into running fp64 sums, maxima and int64 counts
//   batch_stats_kernel      [mean reward, mean reset, mean terminal, max reward] over T*B elements (reset counted in integers)
//   masked_mean_kernel      the mean over the first take_rows rows of the kept columns, with or without skipping NaNs
//   export_image_u8_kernel  (T,B,C,H,W) float -> (take_b,T,H,W,C) uint8, clip((x + 0.5) * 255) in fp32 without contraction
#include "common.h"

namespace {

constexpr int LG_THREADS = 256;

// the block's sum of v in a fixed tree; every thread calls it; the result is valid in every thread
__device__ __forceinline__ double lg_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();      // red may still be read from the previous call
  red[t] = v;
  __syncthreads();
  for (int s = LG_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ long long lg_block_sum_i(long long v, long long* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = LG_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// torch.max's rule: a NaN wins
__device__ __forceinline__ float lg_max_nan(float a, float b) { return (isnan(a) || isnan(b)) ? NAN : fmaxf(a, b); }

__device__ __forceinline__ float lg_block_max_nan(float v, float* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = LG_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = lg_max_nan(red[t], red[t + s]);
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(LG_THREADS) metric_accum_kernel(int n, const float* __restrict__ vals,
                                                                  const unsigned char* __restrict__ rules, double* __restrict__ sum,
                                                                  double* __restrict__ maxv, long long* __restrict__ count) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const int rule = rules[i];
  if (rule < 1 || rule > 4) return;
  const float v = vals[i];
  const bool counted = rule == 1 ? !isnan(v) : rule == 2 ? isfinite(v) : rule == 3;
  if (counted) {
    sum[i] += (double)v;
    count[i] += 1;
  }
  if ((rule == 2 && counted) || rule == 4) {
    const double m = maxv[i], d = (double)v;
    maxv[i] = (isnan(m) || isnan(d)) ? (double)NAN : (d > m ? d : m);
  }
}

__global__ void __launch_bounds__(LG_THREADS) batch_stats_kernel(int n, const float* __restrict__ reward,
                                                                 const unsigned char* __restrict__ reset,
                                                                 const float* __restrict__ terminal, float* __restrict__ out4) {
  __shared__ double red[LG_THREADS];
  __shared__ long long redi[LG_THREADS];
  __shared__ float redm[LG_THREADS];
  const int t = threadIdx.x;
  double sr = 0.0, st = 0.0;
  long long cr = 0;
  float mx = -INFINITY;
  for (int i = t; i < n; i += LG_THREADS) {
    const float r = reward[i];
    sr += (double)r;
    mx = lg_max_nan(mx, r);
    cr += reset[i] ? 1 : 0;
    if (terminal) st += (double)terminal[i];
  }
  sr = lg_block_sum(sr, red);
  st = lg_block_sum(st, red);
  cr = lg_block_sum_i(cr, redi);
  mx = lg_block_max_nan(mx, redm);
  if (t == 0) {
    out4[0] = (float)(sr / (double)n);
    out4[1] = (float)cr / (float)n;
    out4[2] = terminal ? (float)(st / (double)n) : 0.f;
    out4[3] = mx;
  }
}

__global__ void __launch_bounds__(LG_THREADS) masked_mean_kernel(int rows, int B, const float* __restrict__ x, int ldx,
                                                                 const unsigned char* __restrict__ col_keep, int skip_nan,
                                                                 float* __restrict__ out) {
  __shared__ double red[LG_THREADS];
  __shared__ long long redi[LG_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  long long c = 0;
  const int total = rows * B;      // host-checked: fits an int
  for (int i = t; i < total; i += LG_THREADS) {
    const int r = i / B, b = i - r * B;
    if (col_keep && !col_keep[b]) continue;
    const float v = x[(size_t)r * ldx + b];
    if (skip_nan && isnan(v)) continue;
    s += (double)v;
    c += 1;
  }
  s = lg_block_sum(s, red);
  c = lg_block_sum_i(c, redi);
  if (t == 0) out[0] = c > 0 ? (float)(s / (double)c) : NAN;
}

__global__ void __launch_bounds__(LG_THREADS) export_image_u8_kernel(int T, int B, int nb, int C, int H, int W,
                                                                     const float* __restrict__ src, unsigned char* __restrict__ dst) {
  const long long hw = (long long)H * W, total = (long long)nb * T * hw * C;
  const long long stride = (long long)gridDim.x * LG_THREADS;
  for (long long o = (long long)blockIdx.x * LG_THREADS + threadIdx.x; o < total; o += stride) {      // o walks dst (b, t, h, w, c)
    long long q = o;
    const int c = (int)(q % C); q /= C;
    const long long p = q % hw; q /= hw;
    const int t = (int)(q % T);
    const int b = (int)(q / T);
    const float x = src[(((long long)t * B + b) * C + c) * hw + p];
    const float y = __fmul_rn(__fadd_rn(x, 0.5f), 255.0f);
    dst[o] = (unsigned char)(int)(y > 0.f ? (y < 255.f ? y : 255.f) : 0.f);      // NaN fails y > 0: gives 0
  }
}

}  // namespace

extern "C" int dm_metric_accum(int n, const float* vals, const uint8_t* rules, double* sum, double* maxv, int64_t* count,
                               void* stream) {
  DM_REQUIRE(vals && rules && sum && maxv && count, DM_E_NULL, "metric_accum: null pointer");
  DM_REQUIRE(n >= 1 && n <= LG_THREADS, DM_E_SHAPE, "metric_accum: n=%d (1 ... %d)", n, LG_THREADS);
  hipLaunchKernelGGL(metric_accum_kernel, dim3(1), dim3(LG_THREADS), 0, (hipStream_t)stream, n, vals, rules, sum, maxv,
                     (long long*)count);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_batch_stats(int n, const float* reward, const uint8_t* reset, const float* terminal, float* out4, void* stream) {
  DM_REQUIRE(reward && reset && out4, DM_E_NULL, "batch_stats: null pointer");      // terminal may be NULL
  DM_REQUIRE(n >= 1 && n <= (1 << 24), DM_E_SHAPE, "batch_stats: n=%d (1 ... 2^24: one workgroup walks it)", n);
  hipLaunchKernelGGL(batch_stats_kernel, dim3(1), dim3(LG_THREADS), 0, (hipStream_t)stream, n, reward, reset, terminal, out4);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_masked_mean(int T, int B, const float* x, int ldx, int take_rows, const uint8_t* col_keep, int skip_nan,
                              float* out, void* stream) {
  DM_REQUIRE(x && out, DM_E_NULL, "masked_mean: null pointer");      // col_keep may be NULL
  DM_REQUIRE(T >= 1 && B >= 1 && take_rows >= 1, DM_E_SHAPE, "masked_mean: T=%d B=%d take_rows=%d", T, B, take_rows);
  DM_REQUIRE(ldx >= B, DM_E_SHAPE, "masked_mean: ldx=%d below B=%d", ldx, B);
  DM_REQUIRE(skip_nan == 0 || skip_nan == 1, DM_E_SHAPE, "masked_mean: skip_nan=%d", skip_nan);
  const int rows = take_rows < T ? take_rows : T;
  DM_REQUIRE((int64_t)rows * B <= (1 << 24), DM_E_SHAPE, "masked_mean: %d rows x %d columns (up to 2^24 elements)", rows, B);
  hipLaunchKernelGGL(masked_mean_kernel, dim3(1), dim3(LG_THREADS), 0, (hipStream_t)stream, rows, B, x, ldx, col_keep, skip_nan, out);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_export_image_u8(int T, int B, int take_b, int C, int H, int W, const float* src, uint8_t* dst, void* stream) {
  DM_REQUIRE(src && dst, DM_E_NULL, "export_image_u8: null pointer");
  DM_REQUIRE(T >= 1 && B >= 1 && take_b >= 1 && H >= 1 && W >= 1, DM_E_SHAPE, "export_image_u8: T=%d B=%d take_b=%d H=%d W=%d", T, B,
             take_b, H, W);
  DM_REQUIRE(C == 1 || C == 3, DM_E_SHAPE, "export_image_u8: C=%d (1 or 3: grayscale or RGB)", C);
  DM_REQUIRE(H == W, DM_E_SHAPE, "export_image_u8: H=%d W=%d (square images only, as train.py:446-448)", H, W);
  DM_REQUIRE((int64_t)T * B * C * H * W <= ((int64_t)1 << 28), DM_E_SHAPE, "export_image_u8: %lld elements (up to 2^28)",
             (long long)T * B * C * H * W);
  const int nb = take_b < B ? take_b : B;
  const int64_t total = (int64_t)nb * T * C * H * W;      // elementwise, so a grid: a logged Atari batch is 30 M pixels
  const int blocks = total < (int64_t)LG_THREADS * 1024 ? dm_cdiv(total, LG_THREADS) : 1024;
  hipLaunchKernelGGL(export_image_u8_kernel, dim3(blocks), dim3(LG_THREADS), 0, (hipStream_t)stream, T, B, nb, C, H, W, src, dst);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
