// The two-hot symlog critic and the percentile return normalisation (DreamerV3's critic head and advantage scaling; the reference
// has no counterpart).  fp32 throughout, no float atomics, no scratch memory, every float sum in a fixed order: the same inputs
// give the same bits.
//
//   twohot_kernel<KP, E>   KP lanes per row (a power of two, 2 .. 64), E elements per lane: lane l of a row group holds the logits
//                          and bins j = l + e KP, e = 0 .. E-1 (K <= KP E; consecutive lanes read consecutive floats).  64 / KP rows
//                          per wave, 256 / KP rows per block - cat_support.hip's scheme carried to K <= 256.  Per row, in this order:
//     m      = max_j logit_j                      (lane-local over e ascending, then an xor-butterfly over the KP lanes)
//     e_j    = expf(logit_j - m);  s = sum_j e_j  (lane-local over e ascending, then the butterfly);  p_j = e_j / s
//     mu     = sum_j fl(p_j bins_j)               (the same order);  value = symexp(mu) = copysign(expm1f(|mu|), mu)
//     x      = min(max(symlog(target), bins_0), bins_{K-1}),  symlog(t) = copysign(log1pf(|t|), t)
//     k      = min(max(#{i : bins_i <= x} - 1, 0), K - 2)     (integer counts: exact, order-free)
//     w_hi   = fl(fl(x - bins_k) / fl(bins_{k+1} - bins_k));  w_lo = fl(1 - w_hi)
//     lse    = fl(m + logf(s))
//     loss   = fl(weight fl(fl(lse - fl(w_lo logit_k)) - fl(w_hi logit_{k+1})))
//     dlogit_j = fl(fl(scale weight) fl(p_j - y_j)),  y_k = w_lo, y_{k+1} = w_hi, 0 elsewhere
//                          Rows [rows, rows_total) of dlogits are stored as zeros by the same launch.  The lanes j >= K carry logit
//                          -inf (probability exactly 0) and bin 0: they never win a reduction and store nothing.  A NaN target
//                          counts no bin and lands on k = 0: every index stays inside the row.
//                          The head form (dm_twohot_head_loss) runs the same instances with tdiv = I and weight = NULL: row r reads
//                          target[r / I], and the weight is the constant 1.0f (fl(1 x) = x: the bits of the line above with
//                          weight = 1); there loss may be NULL too.
//   return_norm_select_kernel   ONE workgroup of 1024 threads.  The order statistics s_i of the n values are found by an exact
//                          radix select over the order-preserving integer image of the float (sign bit flipped for x >= 0, all
//                          bits for x < 0; -0 sorts below +0): four passes of 8 bits, most significant first, each a histogram
//                          of the digit over the values that share the rank's prefix (LDS integer adds: exact, order-free), then a
//                          wave prefix scan picks the digit.  The four ranks i_lo, i_lo + 1, i_hi, i_hi + 1 walk together and
//                          share a histogram while their prefixes agree.  Then thread 0, for q in (q_lo, q_hi):
//     pos = fl(q fl(n - 1));  i = floor(pos);  fr = fl(pos - i);  p = fl(s_i + fl(fr fl(s_{i+1} - s_i)))      (s_n read as s_{n-1})
//     update != 0:  state_c = fl(fl(decay state_c) + fl(fl(1 - decay) p_c))      for c = lo, hi
//     scale = max(limit, fl(hi - lo));  out = [p_lo, p_hi, lo, hi, scale]
//   return_norm_scale_kernel    adv_i = fl(adv_i / scale) with the scale read from out[4] (IEEE division).
#include "common.h"

#include <math.h>

// Every product and sum of this file is rounded on its own, as the text above counts them (cem.hip has the reasoning).
#pragma clang fp contract(off)

namespace {

constexpr int TH_THREADS = 256;
constexpr int RN_THREADS = 1024;

__device__ __forceinline__ float symlog(float t) { return copysignf(log1pf(fabsf(t)), t); }
__device__ __forceinline__ float symexp(float m) { return copysignf(expm1f(fabsf(m)), m); }

template <int KP, int E>
__global__ void __launch_bounds__(TH_THREADS) twohot_kernel(int rows, int rows_total, int K, const float* __restrict__ logits, int ld,
                                                            const float* __restrict__ bins, const float* __restrict__ target,
                                                            const float* __restrict__ weight, float scale, float* __restrict__ loss,
                                                            float* __restrict__ dlogits, float* __restrict__ value, int tdiv) {
  constexpr int RPB = TH_THREADS / KP;
  const int l = threadIdx.x & (KP - 1);
  const long long r = (long long)blockIdx.x * RPB + (threadIdx.x / KP);
  const bool row_ok = r < rows;
  float x[E], b[E];
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = l + e * KP;
    const bool live = row_ok && j < K;
    b[e] = j < K ? bins[j] : 0.f;
    x[e] = live ? logits[(size_t)r * ld + j] : -INFINITY;
    m = fmaxf(m, x[e]);
  }
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, KP));
  // a row outside the matrix has m = -inf: its lanes compute NaN and store nothing but the zero tail of dlogits
  float p[E];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    p[e] = (l + e * KP < K) ? expf(x[e] - m) : 0.f;
    s += p[e];
  }
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, KP);
  float mu = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    p[e] = p[e] / s;
    mu += p[e] * b[e];
  }
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) mu += __shfl_xor(mu, o, KP);
  if (value && row_ok && l == 0) value[r] = symexp(mu);
  if (!target) return;      // the decode form (uniform over the grid)
  if (!row_ok) {            // the rows behind the loss rows: no gradient (uniform over the lane group)
    if (dlogits && r < rows_total) {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (l + e * KP < K) dlogits[(size_t)r * K + l + e * KP] = 0.f;
    }
    return;
  }
  const float b0 = bins[0], b1 = bins[K - 1];
  const float xt = fminf(fmaxf(symlog(target[tdiv > 1 ? r / tdiv : r]), b0), b1);
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) cnt += (l + e * KP < K && b[e] <= xt) ? 1 : 0;
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, KP);
  const int k = min(max(cnt - 1, 0), K - 2);
  const float bk = bins[k], bk1 = bins[k + 1];
  const float w_hi = (xt - bk) / (bk1 - bk), w_lo = 1.f - w_hi;
  const float w = weight ? weight[r] : 1.f;
  if (dlogits) {
    const float sw = scale * w;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = l + e * KP;
      if (j < K) dlogits[(size_t)r * K + j] = sw * (p[e] - (j == k ? w_lo : (j == k + 1 ? w_hi : 0.f)));
    }
  }
  if (l == 0 && loss) {
    const float lk = logits[(size_t)r * ld + k], lk1 = logits[(size_t)r * ld + k + 1];
    const float lse = m + logf(s);
    loss[r] = w * ((lse - w_lo * lk) - w_hi * lk1);
  }
}

template <int KP, int E>
void launch(int rows, int rows_total, int K, const float* logits, int ld, const float* bins, const float* target, const float* weight,
            float scale, float* loss, float* dlogits, float* value, int tdiv, hipStream_t st) {
  const int cover = dlogits ? rows_total : rows;
  hipLaunchKernelGGL((twohot_kernel<KP, E>), dim3(dm_cdiv(cover, TH_THREADS / KP)), dim3(TH_THREADS), 0, st, rows, rows_total, K,
                     logits, ld, bins, target, weight, scale, loss, dlogits, value, tdiv);
}

void dispatch(int rows, int rows_total, int K, const float* logits, int ld, const float* bins, const float* target,
              const float* weight, float scale, float* loss, float* dlogits, float* value, int tdiv, hipStream_t st) {
#define TH_GO(KP, E) launch<KP, E>(rows, rows_total, K, logits, ld, bins, target, weight, scale, loss, dlogits, value, tdiv, st)
  if (K <= 2) TH_GO(2, 1);
  else if (K <= 4) TH_GO(4, 1);
  else if (K <= 8) TH_GO(8, 1);
  else if (K <= 16) TH_GO(16, 1);
  else if (K <= 32) TH_GO(32, 1);
  else if (K <= 64) TH_GO(64, 1);
  else if (K <= 128) TH_GO(64, 2);
  else TH_GO(64, 4);
#undef TH_GO
}

// order-preserving image of a float: a < b as floats (with -0 < +0) <=> key(a) < key(b) as unsigned integers
__device__ __forceinline__ unsigned rn_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rn_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ void __launch_bounds__(RN_THREADS) return_norm_select_kernel(int n, const float* __restrict__ x, float q_lo, float q_hi,
                                                                        float decay, float limit, int update,
                                                                        float* __restrict__ state, float* __restrict__ out) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned prefix[4], rem[4], dprefix[4];
  __shared__ int hsel[4], nd_s;
  __shared__ float fr_s[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    const float nm1 = (float)(n - 1);
    const float qs[2] = {q_lo, q_hi};
    for (int c = 0; c < 2; ++c) {
      const float pos = qs[c] * nm1;
      int i = (int)floorf(pos);
      i = min(max(i, 0), n - 1);      // (a NaN q never gets here: the host refuses it)
      fr_s[c] = pos - (float)i;
      rem[2 * c] = (unsigned)i;
      rem[2 * c + 1] = (unsigned)min(i + 1, n - 1);
    }
    for (int j = 0; j < 4; ++j) prefix[j] = 0u;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    __syncthreads();
    if (tid == 0) {      // ranks whose prefixes agree share one histogram
      int nd = 0;
      for (int j = 0; j < 4; ++j) {
        int h = -1;
        for (int d = 0; d < nd; ++d)
          if (dprefix[d] == prefix[j]) { h = d; break; }
        if (h < 0) { h = nd; dprefix[nd++] = prefix[j]; }
        hsel[j] = h;
      }
      nd_s = nd;
    }
    for (int e = tid; e < 4 * 256; e += RN_THREADS) (&hist[0][0])[e] = 0u;
    __syncthreads();
    const int nd = nd_s;
    const unsigned dp0 = dprefix[0], dp1 = dprefix[1], dp2 = dprefix[2], dp3 = dprefix[3];
    for (int i = tid; i < n; i += RN_THREADS) {
      const unsigned key = rn_key(x[i]);
      const unsigned hi = pass == 0 ? 0u : key >> (shift + 8);
      const unsigned digit = (key >> shift) & 255u;
      if (hi == dp0) atomicAdd(&hist[0][digit], 1u);
      if (nd > 1 && hi == dp1) atomicAdd(&hist[1][digit], 1u);
      if (nd > 2 && hi == dp2) atomicAdd(&hist[2][digit], 1u);
      if (nd > 3 && hi == dp3) atomicAdd(&hist[3][digit], 1u);
    }
    __syncthreads();
    if (wave < 4) {      // wave j settles rank j: the digit d with cum(d - 1) <= rem < cum(d)
      const int j = wave, h = hsel[j];
      const unsigned want = rem[j];
      const unsigned c0 = hist[h][4 * lane], c1 = hist[h][4 * lane + 1], c2 = hist[h][4 * lane + 2], c3 = hist[h][4 * lane + 3];
      const unsigned c = c0 + c1 + c2 + c3;
      unsigned inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      const unsigned exc = inc - c;
      const bool mine = want >= exc && want < inc;
      const unsigned long long found = __ballot(mine);
      if (mine) {
        unsigned rr = want - exc;
        int d = 0;
        if (rr >= c0) { rr -= c0; d = 1;
          if (rr >= c1) { rr -= c1; d = 2;
            if (rr >= c2) { rr -= c2; d = 3; } } }
        prefix[j] = (prefix[j] << 8) | (unsigned)(4 * lane + d);
        rem[j] = rr;
      } else if (found == 0ull && lane == 63) {      // unreachable while the counts add up to n; keeps the walk defined
        prefix[j] = (prefix[j] << 8) | 255u;
        rem[j] = 0u;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    float p[2];
    for (int c = 0; c < 2; ++c) {
      const float s0 = rn_unkey(prefix[2 * c]), s1 = rn_unkey(prefix[2 * c + 1]);
      p[c] = s0 + fr_s[c] * (s1 - s0);
    }
    float lo = state[0], hi = state[1];
    if (update) {
      const float om = 1.f - decay;
      lo = decay * lo + om * p[0];
      hi = decay * hi + om * p[1];
      state[0] = lo;
      state[1] = hi;
    }
    out[0] = p[0];
    out[1] = p[1];
    out[2] = lo;
    out[3] = hi;
    out[4] = fmaxf(limit, hi - lo);
  }
}

__global__ void __launch_bounds__(256) return_norm_scale_kernel(int n_adv, const float* __restrict__ out, float* __restrict__ adv) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_adv) adv[i] = adv[i] / out[4];
}

int twohot_checks(const char* who, int rows, int rows_total, int K, const float* logits, int ld, const float* bins) {
  DM_REQUIRE(K >= 2 && K <= 256, DM_E_SHAPE, "%s: K=%d (2 .. 256 bins)", who, K);
  DM_REQUIRE(rows >= 0 && rows_total >= rows, DM_E_SHAPE, "%s: rows=%d rows_total=%d", who, rows, rows_total);
  DM_REQUIRE(ld >= K, DM_E_SHAPE, "%s: ld=%d < K=%d", who, ld, K);
  DM_REQUIRE(logits && bins, DM_E_NULL, "%s: null logits or bins", who);
  return DM_OK;
}

}  // namespace

extern "C" int dm_twohot_decode(int rows, int K, const float* logits, int ld, const float* bins, float* value, void* stream) {
  DM_TRY(twohot_checks("twohot_decode", rows, rows, K, logits, ld, bins));
  DM_REQUIRE(value, DM_E_NULL, "twohot_decode: null value");
  if (rows <= 0) return DM_OK;
  dispatch(rows, rows, K, logits, ld, bins, nullptr, nullptr, 0.f, nullptr, nullptr, value, 1, (hipStream_t)stream);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_twohot_loss(int rows, int rows_total, int K, const float* logits, int ld, const float* bins, const float* target,
                              const float* weight, float scale, float* loss, float* dlogits, float* value, void* stream) {
  DM_TRY(twohot_checks("twohot_loss", rows, rows_total, K, logits, ld, bins));
  DM_REQUIRE(target && weight && loss, DM_E_NULL, "twohot_loss: null target, weight or loss");
  if ((dlogits ? rows_total : rows) <= 0) return DM_OK;
  dispatch(rows, rows_total, K, logits, ld, bins, target, weight, scale, loss, dlogits, value, 1, (hipStream_t)stream);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

// The head form of dm_twohot_loss: rows = (t, b, i) rows of a decoder head under iwae_samples = I, row r against target[r / I], no
// weight array (weight 1), every output optional, target == NULL the mean-only form (dm_twohot_decode's bits).  One launch.
extern "C" int dm_twohot_head_loss(int rows, int I, int K, const float* logits, int ld, const float* bins, const float* target,
                                   float scale, float* loss, float* dlogits, float* mean, void* stream) {
  DM_TRY(twohot_checks("twohot_head_loss", rows, rows, K, logits, ld, bins));
  DM_REQUIRE(I >= 1 && rows % I == 0, DM_E_SHAPE, "twohot_head_loss: rows=%d I=%d (I >= 1, rows a multiple of I)", rows, I);
  DM_REQUIRE(target || (!loss && !dlogits), DM_E_NULL, "twohot_head_loss: loss or dlogits asked for without a target");
  DM_REQUIRE(loss || dlogits || mean, DM_E_NULL, "twohot_head_loss: no output");
  if (rows <= 0) return DM_OK;
  dispatch(rows, rows, K, logits, ld, bins, target, nullptr, scale, loss, dlogits, mean, I, (hipStream_t)stream);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_return_norm(int n, const float* x, float q_lo, float q_hi, float decay, float limit, int update, float* state,
                              float* out, float* adv, int n_adv, void* stream) {
  DM_REQUIRE(n >= 1 && n_adv >= 0, DM_E_SHAPE, "return_norm: n=%d n_adv=%d", n, n_adv);
  DM_REQUIRE(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, DM_E_SHAPE, "return_norm: q_lo=%g q_hi=%g (0 <= q_lo <= q_hi <= 1)", q_lo, q_hi);
  DM_REQUIRE(decay >= 0.f && decay < 1.f, DM_E_SHAPE, "return_norm: decay=%g (0 <= decay < 1)", decay);
  DM_REQUIRE(limit > 0.f && limit <= 3.402823466e38f, DM_E_SHAPE, "return_norm: limit=%g (finite, > 0)", limit);
  DM_REQUIRE(x && state && out, DM_E_NULL, "return_norm: null x, state or out");
  DM_REQUIRE(adv || n_adv == 0, DM_E_NULL, "return_norm: null adv with n_adv=%d", n_adv);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(return_norm_select_kernel, dim3(1), dim3(RN_THREADS), 0, st, n, x, q_lo, q_hi, decay, limit, update, state, out);
  if (n_adv > 0) hipLaunchKernelGGL(return_norm_scale_kernel, dim3(dm_cdiv(n_adv, 256)), dim3(256), 0, st, n_adv, out, adv);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
