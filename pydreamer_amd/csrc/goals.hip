// The goals probe's metric arithmetic (probes.py:113-135): over rows = T*B frames and G goals,
//   mse_goals         = mean over (row, goal) of dx^2 + dy^2, coordinates (2g, 2g+1) of a 2G-wide row belong to goal g,
//   var_goals         = (1/G) sum over the 2G coordinates of the UNBIASED variance of that coordinate over the rows,
//   mse_goal_age{..}  = per age bucket, the mean of dx^2 + dy^2 over the (row, goal) entries whose `visage` lies in the bucket.
// A 2G-wide row is a few cache lines, so the lanes of a 64-wide wave run over ROWS and every wave owns a contiguous run of
// 64*k rows (k = 1 up to 65 536 rows: at most GS_MAX_WAVES waves).  Three launches, no float atomics, every sum in a fixed order
// (a lane's rows in sequence, the xor butterfly of the wave, then the waves in sequence): the same inputs give the same bits.
//   1  goals_partial_kernel   per wave: the sums of the 2G coordinates, of the squared errors, and the 6 bucket sums / counts
//   2  goals_center_kernel    every block adds the coordinate sums of all waves (same order in every block: same means),
//                             then per wave: sum (x - mean)^2 - the two-pass variance; no  sum x^2 - n mean^2  anywhere
//   3  goals_final_kernel     one block: the waves' partials in sequence, the divisions, the scalars into the caller's slots
// The variance of one row is 0 / 0 = NaN and an empty bucket's mean is 0 / 0 = NaN, as torch's var() and the reference's
// nanmean(x * mask / mask) give.  Ages are compared as floats against the inclusive bounds [0,0] [1,5] [6,10] [11,50] [51,200]
// [201,1000]: 0.5 or 5.5 falls between two buckets, a negative age or one above 1000 in none.
#include "common.h"

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int GS_MAX_WAVES = 1024;
constexpr int GS_BUCKETS = 6;
constexpr int GS_HEAD = 1 + 2 * GS_BUCKETS;      // per-wave record: [0] sum of squared errors, [1..6] bucket sums, [7..12] bucket counts (int bits)

// per-wave record of the workspace: GS_HEAD + 2G coordinate sums + 2G centred square sums
__host__ __device__ __forceinline__ int gs_stride(int G) { return GS_HEAD + 4 * G; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int age_bucket(float a) {
  if (a == 0.f) return 0;
  if (a >= 1.f && a <= 5.f) return 1;
  if (a >= 6.f && a <= 10.f) return 2;
  if (a >= 11.f && a <= 50.f) return 3;
  if (a >= 51.f && a <= 200.f) return 4;
  if (a >= 201.f && a <= 1000.f) return 5;
  return -1;      // NaN, negative, non-integer between two buckets, above 1000 (1e5: never seen)
}

__global__ void __launch_bounds__(GS_THREADS) goals_partial_kernel(int rows, int G, int rpw, int nwaves, const float* __restrict__ goals,
                                                                   const float* __restrict__ pred, const float* __restrict__ visage,
                                                                   float* __restrict__ ws) {
  const int wave = blockIdx.x * GS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wave >= nwaves) return;      // whole waves leave: the shuffles below see all 64 lanes
  const long long r0 = (long long)wave * rpw;
  const long long r1 = r0 + rpw < rows ? r0 + rpw : rows;
  const int W = 2 * G;
  float* rec = ws + (size_t)wave * gs_stride(G);
  float se = 0.f, bs[GS_BUCKETS];
  int bc[GS_BUCKETS];
#pragma unroll
  for (int b = 0; b < GS_BUCKETS; ++b) { bs[b] = 0.f; bc[b] = 0; }
  for (long long r = r0 + lane; r < r1; r += 64) {
    const float* gr = goals + (size_t)r * W;
    const float* pr = pred + (size_t)r * W;
    for (int g = 0; g < G; ++g) {
      const float dx = gr[2 * g] - pr[2 * g], dy = gr[2 * g + 1] - pr[2 * g + 1];
      const float m = dx * dx + dy * dy;
      se += m;
      if (visage) {
        const int k = age_bucket(visage[(size_t)r * G + g]);
#pragma unroll
        for (int b = 0; b < GS_BUCKETS; ++b)      // static register indices
          if (k == b) { bs[b] += m; bc[b] += 1; }
      }
    }
  }
  se = dm_wave_sum(se);
#pragma unroll
  for (int b = 0; b < GS_BUCKETS; ++b) { bs[b] = dm_wave_sum(bs[b]); bc[b] = wave_sum_i(bc[b]); }
  if (lane == 0) {
    rec[0] = se;
#pragma unroll
    for (int b = 0; b < GS_BUCKETS; ++b) { rec[1 + b] = bs[b]; rec[1 + GS_BUCKETS + b] = __int_as_float(bc[b]); }
  }
  for (int j = 0; j < W; ++j) {      // coordinate sums: a row's 2G floats were just read, they come from cache
    float s = 0.f;
    for (long long r = r0 + lane; r < r1; r += 64) s += goals[(size_t)r * W + j];
    s = dm_wave_sum(s);
    if (lane == 0) rec[GS_HEAD + j] = s;
  }
}

__global__ void __launch_bounds__(GS_THREADS) goals_center_kernel(int rows, int G, int rpw, int nwaves, const float* __restrict__ goals,
                                                                  float* __restrict__ ws) {
  extern __shared__ float mean_s[];      // 2G
  const int W = 2 * G, stride = gs_stride(G);
  for (int j = threadIdx.x; j < W; j += GS_THREADS) {
    float s = 0.f;
    for (int w = 0; w < nwaves; ++w) s += ws[(size_t)w * stride + GS_HEAD + j];
    mean_s[j] = s / (float)rows;
  }
  __syncthreads();
  const int wave = blockIdx.x * GS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wave >= nwaves) return;
  const long long r0 = (long long)wave * rpw;
  const long long r1 = r0 + rpw < rows ? r0 + rpw : rows;
  float* rec = ws + (size_t)wave * stride;
  for (int j = 0; j < W; ++j) {
    const float mu = mean_s[j];
    float s = 0.f;
    for (long long r = r0 + lane; r < r1; r += 64) {
      const float d = goals[(size_t)r * W + j] - mu;
      s += d * d;
    }
    s = dm_wave_sum(s);
    if (lane == 0) rec[GS_HEAD + W + j] = s;
  }
}

__global__ void __launch_bounds__(GS_THREADS) goals_final_kernel(int rows, int G, int nwaves, int with_age, const float* __restrict__ ws,
                                                                 float* __restrict__ out) {
  extern __shared__ float var_s[];      // 2G
  const int W = 2 * G, stride = gs_stride(G);
  for (int j = threadIdx.x; j < W; j += GS_THREADS) {
    float s = 0.f;
    for (int w = 0; w < nwaves; ++w) s += ws[(size_t)w * stride + GS_HEAD + W + j];
    var_s[j] = s / (float)(rows - 1);      // torch's default N - 1; one row: 0 / 0 = NaN
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int j = 0; j < W; ++j) v += var_s[j];
    out[1] = v / (float)G;
    float se = 0.f;
    for (int w = 0; w < nwaves; ++w) se += ws[(size_t)w * stride];
    out[0] = se / ((float)rows * (float)G);
  }
  if (with_age && threadIdx.x >= 64 && threadIdx.x < 64 + GS_BUCKETS) {
    const int b = threadIdx.x - 64;
    float s = 0.f;
    long long n = 0;
    for (int w = 0; w < nwaves; ++w) {
      s += ws[(size_t)w * stride + 1 + b];
      n += __float_as_int(ws[(size_t)w * stride + 1 + GS_BUCKETS + b]);
    }
    out[2 + b] = s / (float)n;      // an empty bucket: 0 / 0 = NaN
  }
}

void gs_split(int rows, int* rpw, int* nwaves) {
  const int k = dm_cdiv(rows, 64 * GS_MAX_WAVES);
  *rpw = 64 * (k < 1 ? 1 : k);
  *nwaves = dm_cdiv(rows, *rpw);
}

}  // namespace

extern "C" size_t dm_goals_stats_ws_floats(int rows, int G) {
  if (rows < 1 || G < 1) return 0;
  int rpw, nwaves;
  gs_split(rows, &rpw, &nwaves);
  return (size_t)nwaves * gs_stride(G);
}

extern "C" int dm_goals_stats(int rows, int G, const float* goals, const float* pred, const float* visage, float* out, void* ws,
                              size_t ws_bytes, void* stream) {
  DM_REQUIRE(goals && pred && out, DM_E_NULL, "goals_stats: null pointer");      // visage may be NULL: no age buckets
  DM_REQUIRE(rows >= 0, DM_E_SHAPE, "goals_stats: rows=%d", rows);
  DM_REQUIRE(G >= 1 && G <= 4096, DM_E_SHAPE, "goals_stats: G=%d (1 .. 4096)", G);
  if (rows == 0) return DM_OK;
  const size_t need = dm_goals_stats_ws_floats(rows, G) * sizeof(float);
  DM_REQUIRE(ws, DM_E_NULL, "goals_stats: null workspace");
  DM_REQUIRE(ws_bytes >= need, DM_E_WORKSPACE, "goals_stats: workspace of %zu bytes, need %zu", ws_bytes, need);
  int rpw, nwaves;
  gs_split(rows, &rpw, &nwaves);
  const int blocks = dm_cdiv(nwaves, GS_WAVES);
  const size_t lds = (size_t)2 * G * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(goals_partial_kernel, dim3(blocks), dim3(GS_THREADS), 0, st, rows, G, rpw, nwaves, goals, pred, visage, (float*)ws);
  DM_LAUNCH_CHECK();
  hipLaunchKernelGGL(goals_center_kernel, dim3(blocks), dim3(GS_THREADS), lds, st, rows, G, rpw, nwaves, goals, (float*)ws);
  DM_LAUNCH_CHECK();
  hipLaunchKernelGGL(goals_final_kernel, dim3(1), dim3(GS_THREADS), lds, st, rows, G, nwaves, visage ? 1 : 0, (const float*)ws, out);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
