// Latent-space planning by the cross-entropy method (PlaNet's planner; the reference has no counterpart): the two passes between
// two open-loop rollouts of one CEM iteration.  B environments, J candidates each, Hp steps; M = B J rows, row m = b J + j
// (environment-major, candidate inner); every (Hp, M, ...) array is time-major, the layout dm_rssm_sequence_fwd reads.
//   cem_draw_onehot_kernel      one thread per (t, m).  p = prop[b][t][0 .. A):
//                                 total = p_0 + p_1 + ... + p_{A-1}          (sequential, fp32, k ascending)
//                                 target = fl(u * total)
//                                 cdf_k = cdf_{k-1} + p_k                    (the same chain: cdf_{A-1} has the bits of total)
//                                 idx = #{k : cdf_k <= target}, clamped to A - 1
//                               - dm_sample_onehot's inverse-CDF rule on the probabilities themselves.  The block's indices meet in
//                               LDS and its 256 rows x A one-hot floats leave as one contiguous store.
//   cem_draw_continuous_kernel  one thread per (t, m, a): action = min(max(fl(mean + fl(std * eps)), -1), 1) - the product and the
//                               sum are rounded separately (no fused multiply-add), so the host restates it in two fp32 operations.
//   cem_update_kernel           one workgroup of 256 threads per environment, four stages with a barrier between them; the J
//                               returns (as ranking keys) and the K elite indices stay in LDS.
//     1 returns     thread j, j + 256, ...: g = 1, w = 1, acc = 0; for t = 1 .. Hp in order
//                     acc = fl(acc + fl(fl(g * w) * r_t));  w = fl(w * fl(1 - terminal_t));  g = fl(g * gamma)
//                   then, with a value, acc = fl(acc + fl(fl(g * w) * v)).  g = gamma^(t-1) carries t - 1 roundings, w 2 (t - 1),
//                   a term two more, the sum Hp + 1 adds: |ret - exact| <= (4 Hp + 3) u sum |terms| to first order, u = 2^-24.
//                   ret[m] gets acc as it is; the ranking key is acc, or -FLT_MAX where acc is NaN or +-inf.
//     2 selection   rank_j = #{i : key_i > key_j or (key_i == key_j and i < j)}: J exact comparisons per candidate against the LDS
//                   copy - a permutation of 0 .. J-1 that depends on the keys alone, not on the launch shape.  rank < K: elite[rank] = j.
//     3 refit       kind 0: integer counts cnt[t][a] of the elites' act_idx (LDS integer adds: exact, order-free; an index outside
//                   [0, A) is not counted), freq = fl(cnt / K), mix = alpha pin + (1 - alpha) freq,
//                   pout = (1 - floor) mix + floor / A: at most 8 roundings on non-negative terms.
//                   kinds 1, 2: thread per (t, a): two passes over the K elites in RANK order, each a sequential fp32 sum:
//                   mean_e = fl((x_0 + x_1 + ...) / K), var = fl((d_0^2 + d_1^2 + ...) / K) with d_r = fl(x_r - mean_e),
//                   std_e = sqrtf(var) - the population std from the deviations, never E[x^2] - mean^2;
//                   mean_out = alpha mean_in + (1 - alpha) mean_e, std_out = max(alpha std_in + (1 - alpha) std_e, floor).
//                   prop_in may BE prop_out: every element is read and then written by the same thread, once.
//     4 outputs     first_action = the t = 0 action row of the rank-0 candidate.  Thread 0: stats[0] = key of rank 0, stats[1] =
//                   fl((key_e0 + key_e1 + ...) / K) in rank order, stats[2] = -(sum_a p log p) over prop_out[b][0] with a ascending
//                   (p = 0 adds 0) for kind 0, sum_a logf(std_out[b][0][a]) for kinds 1, 2, stats[3] = prop_out[b][0][executed
//                   class] for kind 0, else 0.
// No float atomics, plain vector stores, every float sum in a fixed order: the same inputs give the same bits.
#include "common.h"
#include <float.h>
#include <limits.h>

// Every product and sum of this file is rounded on its own, as the text above counts them: the compiler's default would fuse
// a * b + c into one rounding (and the _rn intrinsics, inline functions of a header compiled under that default, with it).
#pragma clang fp contract(off)

namespace {

constexpr int CEM_THREADS = 256;
constexpr int CEM_MAX_J = 1024, CEM_MAX_HP = 64, CEM_MAX_A = 64;

__global__ void __launch_bounds__(CEM_THREADS) cem_draw_onehot_kernel(int J, int M, int Hp, int A, const float* __restrict__ prop,
                                                                      const float* __restrict__ u, float* __restrict__ actions,
                                                                      int32_t* __restrict__ act_idx) {
  __shared__ int idx_s[CEM_THREADS];
  const int t = blockIdx.y, m0 = blockIdx.x * CEM_THREADS, m = m0 + threadIdx.x;
  if (m < M) {
    const float* p = prop + ((size_t)(m / J) * Hp + t) * A;
    float total = 0.f;
    for (int k = 0; k < A; ++k) total += p[k];
    const float target = u[(size_t)t * M + m] * total;
    float cdf = 0.f;
    int idx = 0;
    for (int k = 0; k < A; ++k) {
      cdf += p[k];
      idx += (cdf <= target) ? 1 : 0;
    }
    if (idx > A - 1) idx = A - 1;
    idx_s[threadIdx.x] = idx;
    act_idx[(size_t)t * M + m] = idx;
  }
  __syncthreads();
  const int nrows = M - m0 < CEM_THREADS ? M - m0 : CEM_THREADS;
  float* o = actions + ((size_t)t * M + m0) * A;
  for (int e = threadIdx.x; e < nrows * A; e += CEM_THREADS) o[e] = (e % A == idx_s[e / A]) ? 1.f : 0.f;
}

__global__ void __launch_bounds__(CEM_THREADS) cem_draw_continuous_kernel(int J, int M, int Hp, int A, const float* __restrict__ prop,
                                                                          const float* __restrict__ eps, float* __restrict__ actions) {
  const size_t e = (size_t)blockIdx.x * CEM_THREADS + threadIdx.x, n = (size_t)Hp * M * A;
  if (e >= n) return;
  const int a = (int)(e % A);
  const size_t row = e / A;
  const int t = (int)(row / M), m = (int)(row % M);
  const float* p = prop + ((size_t)(m / J) * Hp + t) * 2 * A;
  const float x = p[a] + p[A + a] * eps[e];
  actions[e] = fminf(fmaxf(x, -1.f), 1.f);
}

// prop_in and prop_out may be the same array: no __restrict__ on either
__global__ void __launch_bounds__(CEM_THREADS) cem_update_kernel(int kind, int J, int K, int Hp, int A, float gamma,
                                                                 const float* __restrict__ reward, const float* __restrict__ terminal,
                                                                 const float* __restrict__ value, const float* __restrict__ actions,
                                                                 const int32_t* __restrict__ act_idx, const float* prop_in, float alpha,
                                                                 float floor_, float* prop_out, float* __restrict__ ret,
                                                                 int32_t* __restrict__ elite, float* __restrict__ first_action,
                                                                 float* __restrict__ stats) {
  __shared__ float key_s[CEM_MAX_J];
  __shared__ int elite_s[CEM_MAX_J];
  __shared__ int cnt_s[CEM_MAX_HP * CEM_MAX_A];
  __shared__ float p0_s[CEM_MAX_A];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t M = (size_t)gridDim.x * J, m0 = (size_t)b * J;

  // 1 returns
  for (int j = tid; j < J; j += CEM_THREADS) {
    const size_t m = m0 + j;
    float g = 1.f, w = 1.f, acc = 0.f;
    for (int t = 0; t < Hp; ++t) {
      acc = acc + (g * w) * reward[(size_t)t * M + m];
      w = w * (1.f - terminal[(size_t)t * M + m]);
      g = g * gamma;
    }
    if (value) acc = acc + (g * w) * value[m];
    ret[m] = acc;
    key_s[j] = (acc - acc == 0.f) ? acc : -FLT_MAX;      // NaN and +-inf fail the test
  }
  if (kind == 0)
    for (int e = tid; e < Hp * A; e += CEM_THREADS) cnt_s[e] = 0;
  __syncthreads();

  // 2 selection
  for (int j = tid; j < J; j += CEM_THREADS) {
    const float kj = key_s[j];
    int rank = 0;
    for (int i = 0; i < J; ++i) {
      const float ki = key_s[i];
      rank += (ki > kj || (ki == kj && i < j)) ? 1 : 0;
    }
    if (rank < K) elite_s[rank] = j;
  }
  __syncthreads();
  for (int r = tid; r < K; r += CEM_THREADS) elite[(size_t)b * K + r] = elite_s[r];

  // 3 refit
  if (kind == 0) {
    for (int e = tid; e < Hp * K; e += CEM_THREADS) {
      const int t = e / K, r = e % K;
      const int a = act_idx[(size_t)t * M + m0 + elite_s[r]];
      if (a >= 0 && a < A) atomicAdd(&cnt_s[t * A + a], 1);      // integer, in LDS
    }
    __syncthreads();
    for (int e = tid; e < Hp * A; e += CEM_THREADS) {
      const size_t o = (size_t)b * Hp * A + e;
      const float freq = (float)cnt_s[e] / (float)K;
      const float mix = alpha * prop_in[o] + (1.f - alpha) * freq;
      const float p = (1.f - floor_) * mix + floor_ / (float)A;
      prop_out[o] = p;
      if (e < A) p0_s[e] = p;
    }
  } else {
    for (int e = tid; e < Hp * A; e += CEM_THREADS) {
      const int t = e / A, a = e % A;
      const float* x = actions + ((size_t)t * M + m0) * A + a;
      float s = 0.f;
      for (int r = 0; r < K; ++r) s = s + x[(size_t)elite_s[r] * A];
      const float mean_e = s / (float)K;
      float v = 0.f;
      for (int r = 0; r < K; ++r) {
        const float d = x[(size_t)elite_s[r] * A] - mean_e;
        v = v + d * d;
      }
      const float std_e = sqrtf(v / (float)K);
      const size_t o = ((size_t)b * Hp + t) * 2 * A + a;
      const float mean_in = prop_in[o], std_in = prop_in[o + A];
      const float std_out = fmaxf(alpha * std_in + (1.f - alpha) * std_e, floor_);
      prop_out[o] = alpha * mean_in + (1.f - alpha) * mean_e;
      prop_out[o + A] = std_out;
      if (t == 0) p0_s[a] = std_out;
    }
  }
  __syncthreads();

  // 4 outputs
  const size_t best = m0 + elite_s[0];      // t = 0: row `best` of the first time slice
  for (int a = tid; a < A; a += CEM_THREADS) first_action[(size_t)b * A + a] = actions[best * A + a];
  if (tid == 0) {
    float s = 0.f;
    for (int r = 0; r < K; ++r) s = s + key_s[elite_s[r]];
    float h = 0.f, pa = 0.f;
    if (kind == 0) {
      for (int a = 0; a < A; ++a)
        if (p0_s[a] > 0.f) h -= p0_s[a] * logf(p0_s[a]);
      int a0 = act_idx[best];
      a0 = a0 < 0 ? 0 : (a0 > A - 1 ? A - 1 : a0);
      pa = p0_s[a0];
    } else {
      for (int a = 0; a < A; ++a) h += logf(p0_s[a]);
    }
    float* st = stats + (size_t)b * 4;
    st[0] = key_s[elite_s[0]];
    st[1] = s / (float)K;
    st[2] = h;
    st[3] = pa;
  }
}

int check_sizes(const char* who, int kind, int B, int J, int Hp, int A) {
  DM_REQUIRE(kind >= 0 && kind <= 2, DM_E_SHAPE, "%s: kind %d (0 onehot, 1 tanh_normal, 2 normal_tanh)", who, kind);
  DM_REQUIRE(B >= 1, DM_E_SHAPE, "%s: B=%d", who, B);
  DM_REQUIRE(J >= 1 && J <= CEM_MAX_J, DM_E_SHAPE, "%s: J=%d (1 .. %d candidates)", who, J, CEM_MAX_J);
  DM_REQUIRE(Hp >= 1 && Hp <= CEM_MAX_HP, DM_E_SHAPE, "%s: Hp=%d (1 .. %d steps)", who, Hp, CEM_MAX_HP);
  DM_REQUIRE(A >= 1 && A <= CEM_MAX_A, DM_E_SHAPE, "%s: A=%d (1 .. %d)", who, A, CEM_MAX_A);
  // M = B J as an int, Hp M A / 256 blocks as an int
  DM_REQUIRE((int64_t)B * J <= (int64_t)(INT_MAX / CEM_MAX_HP), DM_E_SHAPE, "%s: B=%d J=%d: B J rows above %d", who, B, J,
             INT_MAX / CEM_MAX_HP);
  return DM_OK;
}

}  // namespace

extern "C" int dm_cem_draw(int kind, int B, int J, int Hp, int A, const float* prop, const float* noise, float* actions,
                           int32_t* act_idx, void* stream) {
  DM_TRY(check_sizes("cem_draw", kind, B, J, Hp, A));
  DM_REQUIRE(prop && noise && actions, DM_E_NULL, "cem_draw: null prop, noise or actions");
  DM_REQUIRE(act_idx || kind != 0, DM_E_NULL, "cem_draw: null act_idx with kind 0");
  const int M = B * J;
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0)
    hipLaunchKernelGGL(cem_draw_onehot_kernel, dim3(dm_cdiv(M, CEM_THREADS), Hp), dim3(CEM_THREADS), 0, st, J, M, Hp, A, prop, noise,
                       actions, act_idx);
  else
    hipLaunchKernelGGL(cem_draw_continuous_kernel, dim3(dm_cdiv((int64_t)Hp * M * A, CEM_THREADS)), dim3(CEM_THREADS), 0, st, J, M, Hp,
                       A, prop, noise, actions);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_cem_update(int kind, int B, int J, int K, int Hp, int A, float gamma, const float* reward, const float* terminal,
                             const float* value, const float* actions, const int32_t* act_idx, const float* prop_in, float alpha,
                             float floor, float* prop_out, float* ret, int32_t* elite, float* first_action, float* stats,
                             void* stream) {
  DM_TRY(check_sizes("cem_update", kind, B, J, Hp, A));
  DM_REQUIRE(K >= 1 && K <= J, DM_E_SHAPE, "cem_update: K=%d (1 .. J=%d elites)", K, J);
  DM_REQUIRE(alpha >= 0.f && alpha <= 1.f, DM_E_SHAPE, "cem_update: alpha=%g (0 .. 1)", (double)alpha);      // NaN fails too
  DM_REQUIRE(floor >= 0.f && (kind != 0 || floor <= 1.f), DM_E_SHAPE, "cem_update: floor=%g (>= 0; kind 0: a share, <= 1)",
             (double)floor);
  DM_REQUIRE(gamma - gamma == 0.f, DM_E_SHAPE, "cem_update: gamma=%g", (double)gamma);
  DM_REQUIRE(reward && terminal && actions && prop_in && prop_out && ret && elite && first_action && stats, DM_E_NULL,
             "cem_update: null pointer");      // value may be NULL
  DM_REQUIRE(act_idx || kind != 0, DM_E_NULL, "cem_update: null act_idx with kind 0");
  hipLaunchKernelGGL(cem_update_kernel, dim3(B), dim3(CEM_THREADS), 0, (hipStream_t)stream, kind, J, K, Hp, A, gamma, reward, terminal,
                     value, actions, act_idx, prop_in, alpha, floor, prop_out, ret, elite, first_action, stats);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
