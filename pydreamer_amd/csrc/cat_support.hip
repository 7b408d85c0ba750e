// The categorical reward head: DenseCategoricalSupportDecoder (decoders.py:322-362) over CategoricalSupport (common.py:77-86).
// A row holds K <= 32 logits over a fixed list of support values; the target's class is the nearest support value, the loss is
// the cross-entropy against it and the decoded value is the probability-weighted mean of the support.
// Layout: KP lanes per row, KP the power of two >= K, so 64 / KP rows per wave and 256 / KP rows per block.  Lane j of a row
// group holds logit j and support value j in registers; with ld == K and KP == K a wave reads one contiguous 64-float piece of
// the logit matrix.  Maximum, sums and the argmin of the squared distance are xor-butterflies inside the KP-lane group: every
// lane of a group ends with the same value, the order of the additions is fixed, there are no atomics and no LDS - the same
// inputs give the same bits.  The lanes j >= K of a group carry logit -inf (probability exactly 0), support 0 and distance
// +inf with an index past every real one: they never win a reduction and store nothing.
// fp32 throughout (expf / logf, the maximum subtracted first), whatever the precision of the products around it.
#include "common.h"

#include <math.h>

namespace {

constexpr int CS_THREADS = 256;

// bin rule (decoders.py:344-347): torch.square(t - sup).argmin(-1) in fp32 - d = t - sup[k], d * d, the first minimum wins
template <int KP>
__global__ void __launch_bounds__(CS_THREADS) head_loss_catsup_kernel(int rows, int I, int K, const float* __restrict__ logits, int ld,
                                                                      const float* __restrict__ support,
                                                                      const float* __restrict__ target, float scale,
                                                                      float* __restrict__ loss, float* __restrict__ dlogits,
                                                                      float* __restrict__ mean_out, int* __restrict__ bin) {
  constexpr int RPB = CS_THREADS / KP;
  const int j = threadIdx.x & (KP - 1);
  const long long r = (long long)blockIdx.x * RPB + (threadIdx.x / KP);
  const bool row_ok = r < rows, live = row_ok && j < K;
  const float sup = j < K ? support[j] : 0.f;
  const float x = live ? logits[(size_t)r * ld + j] : -INFINITY;
  float m = x;
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, KP));
  // a row outside the matrix has m = -inf: its lanes compute NaN and store nothing
  const float e = j < K ? expf(x - m) : 0.f;
  float s = e;
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, KP);
  const float p = e / s;
  if (mean_out) {
    float mu = p * sup;
#pragma unroll
    for (int o = KP >> 1; o > 0; o >>= 1) mu += __shfl_xor(mu, o, KP);
    if (live && j == 0) mean_out[r] = mu;
  }
  if (!target) return;      // the mean-only form (uniform over the grid)
  const long long g = r / I;
  float dist = INFINITY;
  int best = j < K ? j : KP;
  if (live) {
    const float d = target[g] - sup;
    dist = d * d;
  }
#pragma unroll
  for (int o = KP >> 1; o > 0; o >>= 1) {
    const float od = __shfl_xor(dist, o, KP);
    const int ob = __shfl_xor(best, o, KP);
    // strict '<', the lower index on equal distances; a NaN distance never replaces anything, so lane 0 keeps index 0 when every
    // distance is NaN (torch.argmin of an all-NaN row is 0 too)
    if (od < dist || (od == dist && ob < best)) { dist = od; best = ob; }
  }
  best = __shfl(best, 0, KP);
  const float xb = __shfl(x, best & (KP - 1), KP);
  if (!live) return;
  if (dlogits) dlogits[(size_t)r * K + j] = scale * (p - (j == best ? 1.f : 0.f));
  if (j == 0) {
    if (loss) loss[r] = (m + logf(s)) - xb;
    if (bin && r - g * I == 0) bin[g] = best;
  }
}

template <int KP>
void launch(int rows, int I, int K, const float* logits, int ld, const float* support, const float* target, float scale, float* loss,
            float* dlogits, float* mean_out, int* bin, hipStream_t st) {
  hipLaunchKernelGGL(head_loss_catsup_kernel<KP>, dim3(dm_cdiv(rows, CS_THREADS / KP)), dim3(CS_THREADS), 0, st, rows, I, K, logits, ld,
                     support, target, scale, loss, dlogits, mean_out, bin);
}

}  // namespace

extern "C" int dm_head_loss_catsup(int rows, int I, int K, const float* logits, int ld, const float* support, const float* target,
                                   float scale, float* loss, float* dlogits, float* mean_out, int32_t* bin, void* stream) {
  DM_REQUIRE(K >= 2 && K <= 32, DM_E_SHAPE, "head_loss_catsup: K=%d (2 .. 32 support values)", K);
  DM_REQUIRE(rows >= 0 && I >= 1, DM_E_SHAPE, "head_loss_catsup: rows=%d I=%d", rows, I);
  DM_REQUIRE(rows % I == 0, DM_E_SHAPE, "head_loss_catsup: rows=%d is no multiple of I=%d", rows, I);
  DM_REQUIRE(ld >= K, DM_E_SHAPE, "head_loss_catsup: ld=%d < K=%d", ld, K);
  DM_REQUIRE(logits && support, DM_E_NULL, "head_loss_catsup: null logits or support");
  DM_REQUIRE(target || (!loss && !dlogits && !bin), DM_E_NULL,
             "head_loss_catsup: null target (the mean-only form) with a loss, dlogits or bin output");
  if (rows <= 0) return DM_OK;
  hipStream_t st = (hipStream_t)stream;
  if (K <= 2) launch<2>(rows, I, K, logits, ld, support, target, scale, loss, dlogits, mean_out, bin, st);
  else if (K <= 4) launch<4>(rows, I, K, logits, ld, support, target, scale, loss, dlogits, mean_out, bin, st);
  else if (K <= 8) launch<8>(rows, I, K, logits, ld, support, target, scale, loss, dlogits, mean_out, bin, st);
  else if (K <= 16) launch<16>(rows, I, K, logits, ld, support, target, scale, loss, dlogits, mean_out, bin, st);
  else launch<32>(rows, I, K, logits, ld, support, target, scale, loss, dlogits, mean_out, bin, st);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
