// The acting path's policy draw (generator.py:317-331 restated for B environments): from the actor's output rows and explicit
// noise, ONE call gives the drawn action, its log-probability, the distribution's entropy and the three means the generator logs
// (policy_value, action_prob = mean exp(log_prob), policy_entropy).  Two launches, no float atomics, every sum in a fixed order:
// the same inputs give the same bits.
//   1  policy_draw_onehot_kernel / policy_draw_continuous_kernel   one 64-lane wave per row, lanes over the A classes / action
//                                                                  dimensions (a loop for A > 64); per row exp(log_prob) and the
//                                                                  entropy go to the workspace
//   2  policy_stats_kernel                                         one block: a thread's rows in sequence, then the block's tree
// kind 0 (onehot) draws under the rule of elementwise.hip's sample_onehot kernels with groups = 1, C = A, in their operation order:
//   e_k = expf(x_k - max), sum = e_0 + e_1 + ... (sequential, fp32), p_k = e_k / sum, cdf sequential in k,
//   idx = #{k : cdf_k <= u * cdf_{A-1}} clamped to A - 1
// so the index has the bits dm_sample_onehot gives.  Only the sums that define the rule are sequential (a chain of adds fed by lane
// broadcasts); max is order independent and the entropy is not part of the rule: both use the wave butterfly.
//   log_prob = (x_idx - max) - log(sum),  entropy = -sum_k p_k ((x_k - max) - log(sum))   (a class with p_k = 0 adds 0)
// kinds 1, 2 (tanh_normal, normal_tanh; functions.py:59-78) restate elementwise.hip's sample_continuous kernel: x = mean + std eps,
// action = tanh(x) / x, the same bits.  Both entropies are the base Normal's (functions.py:77).  The log-probability is taken at
// the PRE-tanh draw x - with z = (x - mean) / std = eps, the noise itself, no cancellation - and for kind 1 carries TanhTransform's
// log|det J| = 2 (log 2 - x - softplus(-2 x)) per dimension.  It is NOT recovered from the action through atanh, as the generator's
// log_prob(action) does: near saturation tanh(x) rounds to +-1 and the clamped atanh loses the draw.
// dm_policy_draw_mode: the two draw kernels are templates over the draw mode; MODE 0 is the text above and what dm_policy_draw
// launches, so mode 0 IS dm_policy_draw.
//   MODE 1 (the distribution's mode; no noise is read)  kind 0: idx = the lowest k with x_k == max (a wave min over the lanes' own
//     lowest hit) in place of the CDF walk; kinds 1, 2: eps = 0 through the same expressions - the mode of the BASE Normal pushed
//     through the transform, tanh(5 tanh(m / 5)) / tanh(m), not the best-of-N-samples mode some Dreamer code uses.
//   MODE 2 (sample, then action noise of size amount > 0; amount == 0 is launched as MODE 0)  kind 0: the drawn idx is replaced by
//     min(A - 1, (int)floorf(n2[r][1] * A)) where n2[r][0] < amount, and log_prob is the policy's at the executed index; kinds 1, 2:
//     action = clamp(a + amount n2, -1, 1), log_prob and entropy those of the policy's own draw a.
#include "common.h"

namespace {

constexpr int PD_THREADS = 256;
constexpr int PD_WAVES = PD_THREADS / 64;

// elementwise.hip's dm_sigmoid / dm_softplus / dm_cont_params (file-local there), restated without the derivatives
__device__ __forceinline__ float pd_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float pd_softplus(float v) { return v > 20.f ? v : log1pf(expf(v)); }
__device__ __forceinline__ void pd_cont_params(int kind, float m, float s, float* mean, float* std) {
  if (kind == 1) {
    const float t = tanhf(m / 5.f);
    *mean = 5.f * t;
    *std = pd_softplus(s) + 0.1f;
  } else {
    const float t = tanhf(m);
    *mean = t;
    const float sg = pd_sigmoid(s);
    *std = sg + 0.01f;
  }
}

// rowstat: [0, rows) exp(log_prob), [rows, 2 rows) entropy.  u2, amount: MODE 2 only
template <int MODE>
__global__ void __launch_bounds__(PD_THREADS) policy_draw_onehot_kernel(int rows, int A, const float* __restrict__ logits, int ldp,
                                                                        const float* __restrict__ u, const float* __restrict__ u2,
                                                                        float amount, float* __restrict__ action, int lda,
                                                                        int32_t* __restrict__ act_idx, float* __restrict__ log_prob,
                                                                        float* __restrict__ entropy, float* __restrict__ rowstat) {
  const int row = blockIdx.x * PD_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;      // whole waves leave: the shuffles below see all 64 lanes
  const float* x = logits + (size_t)row * ldp;
  float mx = -INFINITY;
  for (int k = lane; k < A; k += 64) mx = fmaxf(mx, x[k]);
  mx = dm_wave_max(mx);
  float sum = 0.f;
  for (int base = 0; base < A; base += 64) {      // base, n: the same in every lane
    const int k = base + lane, n = A - base < 64 ? A - base : 64;
    const float e = k < A ? expf(x[k] - mx) : 0.f;
    for (int j = 0; j < n; ++j) sum += __shfl(e, j, 64);
  }
  const float lsum = logf(sum);
  float total_p = 0.f, ent = 0.f;
  for (int base = 0; base < A; base += 64) {
    const int k = base + lane, n = A - base < 64 ? A - base : 64;
    const float d = k < A ? x[k] - mx : 0.f;
    const float p = k < A ? expf(d) / sum : 0.f;
    if (MODE != 1)
      for (int j = 0; j < n; ++j) total_p += __shfl(p, j, 64);
    if (p > 0.f) ent -= p * (d - lsum);
  }
  ent = dm_wave_sum(ent);
  int idx = 0;
  if (MODE == 1) {      // the lowest class that holds the maximum: each lane's own lowest hit, then the wave's
    idx = A - 1;        // (a row of NaNs has no hit)
    for (int k = lane; k < A; k += 64)
      if (x[k] == mx) { idx = k; break; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) idx = min(idx, __shfl_xor(idx, off, 64));
  } else {
    const float target = u[row] * total_p;
    float cdf = 0.f;
    for (int base = 0; base < A; base += 64) {
      const int k = base + lane, n = A - base < 64 ? A - base : 64;
      const float p = k < A ? expf(x[k] - mx) / sum : 0.f;
      for (int j = 0; j < n; ++j) {
        cdf += __shfl(p, j, 64);
        idx += (cdf <= target) ? 1 : 0;
      }
    }
    if (idx > A - 1) idx = A - 1;
    if (MODE == 2) {      // row-uniform: every lane reads the same two numbers
      if (u2[(size_t)row * 2] < amount) {
        idx = (int)floorf(u2[(size_t)row * 2 + 1] * (float)A);
        idx = idx > A - 1 ? A - 1 : (idx < 0 ? 0 : idx);
      }
    }
  }
  float* o = action + (size_t)row * lda;
  for (int k = lane; k < A; k += 64) o[k] = (k == idx) ? 1.f : 0.f;
  if (lane == 0) {
    const float lp = (x[idx] - mx) - lsum;
    if (act_idx) act_idx[row] = idx;
    if (log_prob) log_prob[row] = lp;
    if (entropy) entropy[row] = ent;
    rowstat[row] = expf(lp);
    rowstat[(size_t)rows + row] = ent;
  }
}

template <int MODE>
__global__ void __launch_bounds__(PD_THREADS) policy_draw_continuous_kernel(int kind, int rows, int A, const float* __restrict__ params,
                                                                            int ldp, const float* __restrict__ eps,
                                                                            const float* __restrict__ eps2, float amount,
                                                                            float* __restrict__ action, int lda,
                                                                            int32_t* __restrict__ act_idx, float* __restrict__ log_prob,
                                                                            float* __restrict__ entropy, float* __restrict__ rowstat) {
  const float LOG_SQRT_2PI = 0.9189385332046727f;
  const int row = blockIdx.x * PD_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* pr = params + (size_t)row * ldp;
  float lp = 0.f, ent = 0.f;
  for (int a = lane; a < A; a += 64) {
    float mean, std;
    pd_cont_params(kind, pr[a], pr[A + a], &mean, &std);
    const float e = MODE == 1 ? 0.f : eps[(size_t)row * A + a];
    const float x = mean + std * e;
    float act = kind == 1 ? tanhf(x) : x;
    if (MODE == 2) act = fminf(fmaxf(act + amount * eps2[(size_t)row * A + a], -1.f), 1.f);
    action[(size_t)row * lda + a] = act;
    const float ls = logf(std);
    lp += -0.5f * e * e - ls - LOG_SQRT_2PI;
    if (kind == 1) lp -= 2.f * (0.6931471805599453f - x - pd_softplus(-2.f * x));
    ent += 0.5f + LOG_SQRT_2PI + ls;
  }
  lp = dm_wave_sum(lp);
  ent = dm_wave_sum(ent);
  if (lane == 0) {
    if (act_idx) act_idx[row] = 0;
    if (log_prob) log_prob[row] = lp;
    if (entropy) entropy[row] = ent;
    rowstat[row] = expf(lp);
    rowstat[(size_t)rows + row] = ent;
  }
}

__global__ void __launch_bounds__(PD_THREADS) policy_stats_kernel(int rows, const float* __restrict__ rowstat,
                                                                  const float* __restrict__ value, float* __restrict__ stats) {
  __shared__ float red[3][PD_THREADS];
  const int t = threadIdx.x;
  float sp = 0.f, se = 0.f, sv = 0.f;
  for (int r = t; r < rows; r += PD_THREADS) {
    sp += rowstat[r];
    se += rowstat[(size_t)rows + r];
    if (value) sv += value[r];
  }
  red[0][t] = sv; red[1][t] = sp; red[2][t] = se;
  __syncthreads();
  for (int s = PD_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][t] += red[q][t + s];
    }
    __syncthreads();
  }
  if (t < 3) stats[t] = (t == 0 && !value) ? 0.f : red[t][0] / (float)rows;
  if (t == 3) stats[3] = 0.f;
}

}  // namespace

extern "C" size_t dm_policy_draw_ws_floats(int rows) { return rows < 1 ? 0 : (size_t)2 * rows; }

namespace {

template <int MODE>
void policy_draw_launch(int kind, float amount, int rows, int A, const float* params, int ldp, const float* noise, const float* noise2,
                        float* action, int lda, int32_t* act_idx, float* log_prob, float* entropy, float* rowstat, hipStream_t st) {
  const int blocks = dm_cdiv(rows, PD_WAVES);
  if (kind == 0)
    hipLaunchKernelGGL(policy_draw_onehot_kernel<MODE>, dim3(blocks), dim3(PD_THREADS), 0, st, rows, A, params, ldp, noise, noise2,
                       amount, action, lda, act_idx, log_prob, entropy, rowstat);
  else
    hipLaunchKernelGGL(policy_draw_continuous_kernel<MODE>, dim3(blocks), dim3(PD_THREADS), 0, st, kind, rows, A, params, ldp, noise,
                       noise2, amount, action, lda, act_idx, log_prob, entropy, rowstat);
}

// dm_policy_draw is mode 0 of this: its checks, in its order, come first
int policy_draw_impl(int kind, int mode, float amount, int rows, int A, const float* params, int ldp, const float* noise,
                     const float* noise2, const float* value, float* action, int lda, int32_t* act_idx, float* log_prob,
                     float* entropy, float* stats, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(params && (noise || mode == 1) && action && stats, DM_E_NULL, "policy_draw: null pointer");      // value, act_idx, log_prob, entropy may be NULL
  DM_REQUIRE(kind >= 0 && kind <= 2, DM_E_SHAPE, "policy_draw: kind %d (0 onehot, 1 tanh_normal, 2 normal_tanh)", kind);
  DM_REQUIRE(mode >= 0 && mode <= 2, DM_E_SHAPE, "policy_draw: mode %d (0 sample, 1 mode, 2 sample + action noise)", mode);
  DM_REQUIRE(amount >= 0.f, DM_E_SHAPE, "policy_draw: action noise amount %g (must be >= 0)", (double)amount);      // NaN fails too
  DM_REQUIRE(noise2 || !(mode == 2 && amount > 0.f), DM_E_NULL, "policy_draw: null noise2 with action noise %g", (double)amount);
  DM_REQUIRE(rows >= 1 && A >= 1, DM_E_SHAPE, "policy_draw: rows=%d A=%d", rows, A);
  DM_REQUIRE(A <= (1 << 29), DM_E_SHAPE, "policy_draw: A=%d", A);
  const int width = kind == 0 ? A : 2 * A;
  DM_REQUIRE(ldp >= width, DM_E_SHAPE, "policy_draw: ldp=%d below the row width %d", ldp, width);
  DM_REQUIRE(lda >= A, DM_E_SHAPE, "policy_draw: lda=%d below A=%d", lda, A);
  const size_t need = dm_policy_draw_ws_floats(rows) * sizeof(float);
  DM_REQUIRE(ws, DM_E_NULL, "policy_draw: null workspace");
  DM_REQUIRE(ws_bytes >= need, DM_E_WORKSPACE, "policy_draw: workspace of %zu bytes, need %zu", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (mode == 1)
    policy_draw_launch<1>(kind, 0.f, rows, A, params, ldp, nullptr, nullptr, action, lda, act_idx, log_prob, entropy, (float*)ws, st);
  else if (mode == 2 && amount > 0.f)
    policy_draw_launch<2>(kind, amount, rows, A, params, ldp, noise, noise2, action, lda, act_idx, log_prob, entropy, (float*)ws, st);
  else      // mode 0, and mode 2 without noise: the same launch, so the same bits
    policy_draw_launch<0>(kind, 0.f, rows, A, params, ldp, noise, nullptr, action, lda, act_idx, log_prob, entropy, (float*)ws, st);
  DM_LAUNCH_CHECK();
  hipLaunchKernelGGL(policy_stats_kernel, dim3(1), dim3(PD_THREADS), 0, st, rows, (const float*)ws, value, stats);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

}  // namespace

extern "C" int dm_policy_draw(int kind, int rows, int A, const float* params, int ldp, const float* noise, const float* value,
                              float* action, int lda, int32_t* act_idx, float* log_prob, float* entropy, float* stats, void* ws,
                              size_t ws_bytes, void* stream) {
  return policy_draw_impl(kind, 0, 0.f, rows, A, params, ldp, noise, nullptr, value, action, lda, act_idx, log_prob, entropy, stats, ws,
                          ws_bytes, stream);
}

extern "C" int dm_policy_draw_mode(int kind, int mode, float amount, int rows, int A, const float* params, int ldp, const float* noise,
                                   const float* noise2, const float* value, float* action, int lda, int32_t* act_idx, float* log_prob,
                                   float* entropy, float* stats, void* ws, size_t ws_bytes, void* stream) {
  return policy_draw_impl(kind, mode, amount, rows, A, params, ldp, noise, noise2, value, action, lda, act_idx, log_prob, entropy, stats,
                          ws, ws_bytes, stream);
}
