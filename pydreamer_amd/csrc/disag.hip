// Plan2Explore's ensemble kernels (DreamerV2 expl.py: an ensemble of K one-step predictors of the next stochastic state; the
// intrinsic reward is their disagreement).  The heads' outputs are K blocks of (rows, D) with leading dimension ld, the
// blocks head_stride floats apart.
//   disag_reward_kernel   reward[r] = scale * (1/D) sum_d sqrt((1/K) sum_k (x_k - mu)^2), the population std over the heads
//                         (ddof 0, expl.py's std(0)) averaged over the columns.  x_k = m_k - m_0 is exact near a common value
//                         (Sterbenz) and carries only the heads' SPREAD into the sums: a prediction of 1e3 with a spread of
//                         1e-2 keeps its digits, where E[x^2] - mu^2 on the raw values would lose all of them, and K identical
//                         heads give x_k = 0, mu = 0, reward exactly 0.0f.  mu = (sum_k x_k) / K with k ascending.
//                         One wave64 per row: lane l owns the columns l, l + 64, ... in ascending order and keeps the K values
//                         of a column in registers, so for each k the wave reads 256 contiguous bytes; the lanes' sums meet in
//                         the xor butterfly and lane 0 stores.  A lane's columns are 64 floats apart, so its loads are scalar.
//   ensemble_mse_kernel   loss[k][r] = 0.5 sum_d (m_k - y)^2 and dmeans = scale * (m_k - y): the heads' Normal(mean, 1) loss
//                         against the same target row.  One wave64 per (head, row); y is read out of a wider matrix (leading
//                         dimension ldt).  When the row's three addresses are 16-byte aligned the wave walks it as float4
//                         (lane l: columns 4l .. 4l+3, then + 256) and finishes the D % 4 columns one per lane; any other row
//                         is walked one column per lane.  Rows whose skip flag is set store zeros and read nothing.
// Both: fp32 arithmetic whatever the precision of the products around them, one launch, no atomics, every sum in a fixed
// order - the same inputs (at the same addresses) give the same bits.
#include "common.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_WAVES = DG_THREADS / 64;
constexpr int DG_MAX_K = 16;

__global__ void __launch_bounds__(DG_THREADS) disag_reward_kernel(int K, int rows, int D, const float* __restrict__ means,
                                                                  int64_t head_stride, int ld, float scale,
                                                                  float* __restrict__ reward) {
  const long long r = (long long)blockIdx.x * DG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;      // whole waves leave: the shuffles below see all 64 lanes
  const float* row = means + (size_t)r * ld;
  float acc = 0.f;
  for (int d = lane; d < D; d += 64) {
    float x[DG_MAX_K];
#pragma unroll
    for (int k = 0; k < DG_MAX_K; ++k) x[k] = k < K ? row[(size_t)k * head_stride + d] : 0.f;      // static register indices
    const float m0 = x[0];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DG_MAX_K; ++k) {
      x[k] = k < K ? x[k] - m0 : 0.f;
      s += x[k];
    }
    const float mu = s / (float)K;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < DG_MAX_K; ++k) {
      const float c = x[k] - mu;
      if (k < K) v += c * c;
    }
    acc += sqrtf(v / (float)K);
  }
  acc = dm_wave_sum(acc);
  if (lane == 0) reward[r] = scale * (acc / (float)D);
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ void __launch_bounds__(DG_THREADS) ensemble_mse_kernel(int rows, int D, const float* __restrict__ means,
                                                                  int64_t head_stride, int ld, const float* __restrict__ target,
                                                                  int ldt, const uint8_t* __restrict__ skip, float scale,
                                                                  float* __restrict__ loss, float* __restrict__ dmeans) {
  const long long r = (long long)blockIdx.x * DG_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, k = blockIdx.y;
  if (r >= rows) return;
  const size_t off = (size_t)k * head_stride + (size_t)r * ld;
  const float* m = means + off;
  const float* y = target + (size_t)r * ldt;
  float* dm = dmeans ? dmeans + off : nullptr;
  const bool vec = aligned16(m) && aligned16(y) && (!dm || aligned16(dm));      // uniform over the wave
  const int D4 = vec ? (D & ~3) : 0;
  if (skip && skip[r]) {
    if (dm) {
      for (int d = 4 * lane; d < D4; d += 256) *(float4*)(dm + d) = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int d = D4 + lane; d < D; d += 64) dm[d] = 0.f;
    }
    if (lane == 0) loss[(size_t)k * rows + r] = 0.f;
    return;
  }
  float acc = 0.f;
  for (int d = 4 * lane; d < D4; d += 256) {
    const float4 a = *(const float4*)(m + d), b = *(const float4*)(y + d);
    const float4 e = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
    acc += e.x * e.x;
    acc += e.y * e.y;
    acc += e.z * e.z;
    acc += e.w * e.w;
    if (dm) *(float4*)(dm + d) = make_float4(scale * e.x, scale * e.y, scale * e.z, scale * e.w);
  }
  for (int d = D4 + lane; d < D; d += 64) {
    const float e = m[d] - y[d];
    acc += e * e;
    if (dm) dm[d] = scale * e;
  }
  acc = dm_wave_sum(acc);
  if (lane == 0) loss[(size_t)k * rows + r] = 0.5f * acc;
}

int check_heads(const char* who, int K, int rows, int D, int64_t head_stride, int ld) {
  DM_REQUIRE(K >= 2 && K <= DG_MAX_K, DM_E_SHAPE, "%s: K=%d (2 .. %d heads)", who, K, DG_MAX_K);
  DM_REQUIRE(rows >= 0 && D >= 1, DM_E_SHAPE, "%s: rows=%d D=%d", who, rows, D);
  DM_REQUIRE(ld >= D, DM_E_SHAPE, "%s: ld=%d < D=%d", who, ld, D);
  DM_REQUIRE(head_stride >= 0, DM_E_SHAPE, "%s: head_stride=%lld", who, (long long)head_stride);
  return DM_OK;
}

}  // namespace

extern "C" int dm_disag_reward(int K, int rows, int D, const float* means, int64_t head_stride, int ld, float scale,
                               float* reward, void* stream) {
  DM_TRY(check_heads("disag_reward", K, rows, D, head_stride, ld));
  DM_REQUIRE(means && reward, DM_E_NULL, "disag_reward: null means or reward");
  if (rows == 0) return DM_OK;
  hipLaunchKernelGGL(disag_reward_kernel, dim3(dm_cdiv(rows, DG_WAVES)), dim3(DG_THREADS), 0, (hipStream_t)stream, K, rows, D, means,
                     head_stride, ld, scale, reward);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_ensemble_mse(int K, int rows, int D, const float* means, int64_t head_stride, int ld, const float* target,
                               int ldt, const uint8_t* skip, float scale, float* loss, float* dmeans, void* stream) {
  DM_TRY(check_heads("ensemble_mse", K, rows, D, head_stride, ld));
  DM_REQUIRE(ldt >= D, DM_E_SHAPE, "ensemble_mse: ldt=%d < D=%d", ldt, D);
  DM_REQUIRE(means && target && loss, DM_E_NULL, "ensemble_mse: null means, target or loss");      // skip, dmeans may be NULL
  if (rows == 0) return DM_OK;
  hipLaunchKernelGGL(ensemble_mse_kernel, dim3(dm_cdiv(rows, DG_WAVES), K), dim3(DG_THREADS), 0, (hipStream_t)stream, rows, D, means,
                     head_stride, ld, target, ldt, skip, scale, loss, dmeans);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
