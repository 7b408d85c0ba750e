// Per-cell categorical losses over a (C, H, W) logit block: the map probe's CatImageDecoder (decoders.py:183-254) and its
// accuracy (probes.py:73-86).  A row of the MLP's output is class-major, as nn.Unflatten(-1, (C,H,W)) lays it out: the logit
// of class c at cell p sits at c*cells + p, cells = H*W.  The class axis is therefore strided by `cells`, and the kernels put
// the lanes of a 64-wide wave over CELLS: at every class c consecutive lanes read consecutive addresses, and the softmax over
// the classes is a loop inside one lane - no cross-lane traffic until the sum over the cells of a row.  Those sums go through
// a shuffle tree inside the wave and then through LDS across the waves that share a row, always in the same order: no float
// atomics, the same inputs give the same bits.  Everything is fp32 (expf / logf, the maximum subtracted before every exp).
// The path is small (2 500 rows of 1 134 logits at the Atari batch): a row is read two or three times and stays in cache.
#include "common.h"

#include <math.h>

namespace {

constexpr int CI_THREADS = 256;
constexpr int CI_WAVES = CI_THREADS / 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;      // complete in lane 0
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// logsumexp over the classes of one cell: x[c*stride], c < C
__device__ __forceinline__ float cell_lse(const float* __restrict__ x, int C, int stride, float* mx) {
  float m = x[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[(size_t)c * stride]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(x[(size_t)c * stride] - m);
  *mx = m;
  return m + logf(s);
}

// target.argmax(dim=-3) (decoders.py:221): onehot (rows, C, cells) -> idx (rows, cells); strict '>' keeps the lowest class on ties
__global__ void __launch_bounds__(CI_THREADS) cat_target_index_kernel(long long total, int C, int cells,
                                                                      const float* __restrict__ onehot, int* __restrict__ idx) {
  for (long long e = (long long)blockIdx.x * CI_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CI_THREADS) {
    const long long r = e / cells;
    const int p = (int)(e - r * cells);
    const float* x = onehot + (size_t)r * C * cells + p;
    float best = x[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const float v = x[(size_t)c * cells];
      if (v > best) { best = v; bi = c; }
    }
    idx[e] = bi;
  }
}

// One row per group of `wpr` waves (wpr in {1, 2, 4}; CI_WAVES / wpr rows per block).  loss[r] = sum_p (lse_c x - x[target]),
// dlogits = softmax - onehot (decoders.py:227,234).  The target's logit is picked up inside the class loop, so a target
// outside [0, C) reads nothing out of bounds (its cell then contributes the bare logsumexp).
__global__ void __launch_bounds__(CI_THREADS) cat_image_loss_kernel(int rows, int I, int C, int cells, int wpr,
                                                                    const float* __restrict__ logits, int ld,
                                                                    const int* __restrict__ target, float* __restrict__ loss,
                                                                    float* __restrict__ dlogits) {
  __shared__ float part[CI_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rpb = CI_WAVES / wpr;
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
      float z = 0.f, xt = 0.f;
      for (int c = 0; c < C; ++c) {
        const float v = x[(size_t)c * cells + p];
        z += expf(v - m);
        if (c == t) xt = v;
      }
      s += (m + logf(z)) - xt;
      if (d) {
        const float rz = 1.f / z;
        for (int c = 0; c < C; ++c)
          d[(size_t)c * cells + p] = expf(x[(size_t)c * cells + p] - m) * rz - (c == t ? 1.f : 0.f);
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

// One group of I rows per block of `waves` waves; wave w takes the 64-cell chunks w, w + waves, ...  Per cell
// (decoders.py:247-251): lse_i over the classes of every row i, a_c = logsumexp_i (x_ic - lse_i), logp_c = a_c - logsumexp_c a.
// sum_c exp(a_c) = sum_i sum_c softmax_i = I up to rounding, and every a_c <= 0: that last logsumexp needs no maximum.
// lse_i of the chunk in flight is kept in LDS, column `threadIdx.x` of an (I, blockDim.x) array: a lane reads only what it wrote.
__global__ void __launch_bounds__(CI_THREADS) cat_image_pred_kernel(int I, int C, int cells, const float* __restrict__ logits,
                                                                    int ld, const int* __restrict__ target,
                                                                    const int* __restrict__ seen, float* __restrict__ logp,
                                                                    float* __restrict__ acc, float* __restrict__ acc_seen) {
  extern __shared__ float lse_s[];      // (I, blockDim.x)
  __shared__ int cnt[CI_WAVES][3];
  const int g = blockIdx.x, nt = blockDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = nt >> 6;
  const float* x0 = logits + (size_t)g * I * ld;
  int hit = 0, hit_seen = 0, n_seen = 0;
  for (int p = threadIdx.x; p < cells; p += nt) {
    for (int i = 0; i < I; ++i) {
      float m;
      lse_s[i * nt + threadIdx.x] = cell_lse(x0 + (size_t)i * ld + p, C, cells, &m);
    }
    // pass 1: the normaliser over the classes; pass 2: the normalised values, their argmax and the optional store
    float z = 0.f, L = 0.f, best = 0.f;
    int bi = 0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int c = 0; c < C; ++c) {
        const float* xc = x0 + (size_t)c * cells + p;
        float m = xc[0] - lse_s[threadIdx.x];
        for (int i = 1; i < I; ++i) m = fmaxf(m, xc[(size_t)i * ld] - lse_s[i * nt + threadIdx.x]);
        float a = m;
        if (I > 1) {
          float e = 0.f;
          for (int i = 0; i < I; ++i) e += expf((xc[(size_t)i * ld] - lse_s[i * nt + threadIdx.x]) - m);
          a = m + logf(e);
        }
        if (pass == 0) {
          z += expf(a);
        } else {
          const float v = a - L;
          if (c == 0 || v > best) { best = v; bi = c; }      // strict '>': the lowest class wins a tie (torch.argmax)
          if (logp) logp[((size_t)g * C + c) * cells + p] = v;
        }
      }
      if (pass == 0) L = logf(z);
    }
    const int h = bi == target[(size_t)g * cells + p] ? 1 : 0;
    const int sn = seen ? (seen[(size_t)g * cells + p] != 0 ? 1 : 0) : 0;
    hit += h; hit_seen += h & sn; n_seen += sn;
  }
  // counts are integers: exact in any order; the order is fixed all the same (shuffle tree, then the waves in sequence)
  hit = wave_sum_i(hit); hit_seen = wave_sum_i(hit_seen); n_seen = wave_sum_i(n_seen);
  if (lane == 0) { cnt[wave][0] = hit; cnt[wave][1] = hit_seen; cnt[wave][2] = n_seen; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0, b = 0, n = 0;
    for (int w = 0; w < waves; ++w) { a += cnt[w][0]; b += cnt[w][1]; n += cnt[w][2]; }
    if (acc) acc[g] = (float)a / (float)cells;
    if (acc_seen) acc_seen[g] = (float)b / (float)n;      // 0 / 0 = NaN for a frame without a seen cell: nanmean skips it (probes.py:84)
  }
}

// out (rows, F + E) = [ x[r, 0..F) | extra[r / I, 0..E) ]: features with the I-expanded map coordinates behind them (probes.py:54-55)
__global__ void __launch_bounds__(CI_THREADS) cat_concat_rows_kernel(long long total, int I, int F, int E, const float* __restrict__ x,
                                                                     int ldx, const float* __restrict__ extra,
                                                                     float* __restrict__ out) {
  const int W = F + E;
  for (long long e = (long long)blockIdx.x * CI_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CI_THREADS) {
    const long long r = e / W;
    const int j = (int)(e - r * W);
    out[e] = j < F ? x[(size_t)r * ldx + j] : extra[(size_t)(r / I) * E + (j - F)];
  }
}

int ew_grid(long long total) {
  long long b = (total + CI_THREADS - 1) / CI_THREADS;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" int dm_cat_target_index(int rows, int C, int cells, const float* onehot, int32_t* idx, void* stream) {
  DM_REQUIRE(onehot && idx, DM_E_NULL, "cat_target_index: null pointer");
  DM_REQUIRE(C >= 1 && cells >= 1, DM_E_SHAPE, "cat_target_index: C=%d cells=%d", C, cells);
  if (rows <= 0) return DM_OK;
  const long long total = (long long)rows * cells;
  hipLaunchKernelGGL(cat_target_index_kernel, dim3(ew_grid(total)), dim3(CI_THREADS), 0, (hipStream_t)stream, total, C, cells,
                     onehot, idx);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_cat_image_loss(int rows, int I, int C, int cells, const float* logits, int ld, const int32_t* target,
                                 float* loss, float* dlogits, void* stream) {
  DM_REQUIRE(logits && target && loss, DM_E_NULL, "cat_image_loss: null pointer");      // dlogits may be NULL (no backward)
  DM_REQUIRE(C >= 1 && cells >= 1 && I >= 1, DM_E_SHAPE, "cat_image_loss: C=%d cells=%d I=%d", C, cells, I);
  DM_REQUIRE(rows % I == 0, DM_E_SHAPE, "cat_image_loss: rows=%d is no multiple of I=%d", rows, I);
  DM_REQUIRE((long long)ld >= (long long)C * cells, DM_E_SHAPE, "cat_image_loss: ld=%d < C*cells=%lld", ld, (long long)C * cells);
  if (rows <= 0) return DM_OK;
  const int wpr = cells <= 64 ? 1 : (cells <= 128 ? 2 : CI_WAVES);      // waves per row
  const int rpb = CI_WAVES / wpr;
  hipLaunchKernelGGL(cat_image_loss_kernel, dim3(dm_cdiv(rows, rpb)), dim3(CI_THREADS), 0, (hipStream_t)stream, rows, I, C, cells,
                     wpr, logits, ld, target, loss, dlogits);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_cat_image_pred(int groups, int I, int C, int cells, const float* logits, int ld, const int32_t* target,
                                 const int32_t* seen, float* logp, float* acc, float* acc_seen, void* stream) {
  DM_REQUIRE(logits && target && acc, DM_E_NULL, "cat_image_pred: null pointer");      // seen, logp, acc_seen may be NULL
  DM_REQUIRE(!acc_seen || seen, DM_E_NULL, "cat_image_pred: acc_seen without a seen mask");
  DM_REQUIRE(C >= 1 && cells >= 1 && I >= 1, DM_E_SHAPE, "cat_image_pred: C=%d cells=%d I=%d", C, cells, I);
  DM_REQUIRE((long long)ld >= (long long)C * cells, DM_E_SHAPE, "cat_image_pred: ld=%d < C*cells=%lld", ld, (long long)C * cells);
  DM_REQUIRE(I <= 256, DM_E_SHAPE, "cat_image_pred: I=%d (one wave's logsumexp column holds at most 256 samples in 64 KiB of LDS)", I);
  if (groups <= 0) return DM_OK;
  int waves = dm_cdiv(cells, 64);
  if (waves > CI_WAVES) waves = CI_WAVES;
  while (waves > 1 && (size_t)waves * 64 * I * sizeof(float) > 65536) waves >>= 1;
  hipLaunchKernelGGL(cat_image_pred_kernel, dim3(groups), dim3(waves * 64), (size_t)waves * 64 * I * sizeof(float),
                     (hipStream_t)stream, I, C, cells, logits, ld, target, seen, logp, acc, acc_seen);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_cat_concat_rows(int rows, int I, int F, int E, const float* x, int ldx, const float* extra, float* out,
                                  void* stream) {
  DM_REQUIRE(x && extra && out, DM_E_NULL, "cat_concat_rows: null pointer");
  DM_REQUIRE(F >= 1 && E >= 1 && I >= 1 && ldx >= F, DM_E_SHAPE, "cat_concat_rows: F=%d E=%d I=%d ldx=%d", F, E, I, ldx);
  DM_REQUIRE(rows % I == 0, DM_E_SHAPE, "cat_concat_rows: rows=%d is no multiple of I=%d", rows, I);
  if (rows <= 0) return DM_OK;
  const long long total = (long long)rows * (F + E);
  hipLaunchKernelGGL(cat_concat_rows_kernel, dim3(ew_grid(total)), dim3(CI_THREADS), 0, (hipStream_t)stream, total, I, F, E, x, ldx,
                     extra, out);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
