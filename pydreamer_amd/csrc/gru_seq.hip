// Plain GRU over a sequence (torch.nn.GRU, one layer, time-major): the recurrent core of the reference's `gru_probe` baseline
// (pydreamer/models/baselines.py:322,339-341,352 GRUEncoderOnly).  Gate order r, z, n as in torch:
//   GI = X W_ih^T + b_ih                      all T*B rows, one product before the loop
//   GH_t = h_{t-1} W_hh^T + b_hh              per step
//   r = sig(GI_r + GH_r), z = sig(GI_z + GH_z), n = tanh(GI_n + r GH_n), h_t = (h_{t-1} - n) z + n
//
// Forward step, schedule 1 (B <= 64 and 3*D*D < 64K): ONE launch per time step, gru_step_kernel.  A workgroup owns a strip
// of 4 hidden units and 16 batch rows.  The strip's r, z and n rows of W_hh are 12 of the 16 columns of ONE
// v_mfma_f32_16x16x4_f32 tile (the other 4 columns multiply zeros), so the three gate pre-activations of an element end up
// in the same workgroup and the gate arithmetic rides in the epilogue.  The 8 waves split K = D in 16-wide chunks (wave w
// takes chunks w, w + 8, ...) with two independent accumulators per row block, and their partials are summed through LDS
// in wave order: no atomics, the same inputs give the same bits.  D % 4 == 0 makes every strip a full one.
// dm_gru_sequence_fuse_enable(2) dispatches it at every width: how scripts/gru_probe_bench.py and the tests reach it at D >= 148.
// Schedule 0 (wider states, B > 64, or H / W_hh / acts / ws that are not 16-byte aligned): the composed pair, the h W_hh^T product
// through the library's GEMM entry and gru_gates_fwd_kernel - measured faster than the one-launch step at D >= 600, where
// every workgroup of the narrow strips re-reads its rows of h.
//
// Backward: two launches per step (gates backward; dGH_t W_hh + dH_{t-1} accumulated into the carried dh by one product
// with an addend), then the parameter gradients and dX as products over all T*B rows and the bias gradients as column sums.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

static thread_local int tl_gru_sched = 0;
extern "C" int dm_gru_sequence_last_schedule(void) { return tl_gru_sched; }
// 1 (default): the one-launch step where 3*D*D < 64K; 0: never; 2: at every width (benchmark and tests); -1 queries
static int g_gru_fuse = 1;
extern "C" int dm_gru_sequence_fuse_enable(int on) {
  if (on >= 0 && on <= 2) g_gru_fuse = on;
  return g_gru_fuse;
}

constexpr int GS_WAVES = 8;

struct GruStepArgs {
  const float* whh; const float* bhh; const float* gi; const float* hin; int ldhin;
  float* hout; int ldo; float* gh_save; int B, D;
};

__device__ __forceinline__ float gs_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ void __launch_bounds__(GS_WAVES * 64) gru_step_kernel(const GruStepArgs a) {
  constexpr int NRB = 1;      // 16-row blocks per workgroup
  __shared__ float part[GS_WAVES][NRB * 16][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u0 = blockIdx.x * 4, m0 = blockIdx.y * (16 * NRB);
  const int D = a.D;
  // B operand column = lane & 15: gate (col >> 2) of hidden unit u0 + (col & 3); columns 12..15 stay zero
  const int col = lane & 15;
  const bool okb = col < 12;
  const float* wrow = a.whh + (okb ? ((size_t)(col >> 2) * D + u0 + (col & 3)) * D : 0);
  const float* hrow[NRB];
  bool okm[NRB];
#pragma unroll
  for (int mb = 0; mb < NRB; ++mb) {
    const int m = m0 + mb * 16 + (lane & 15);
    okm[mb] = m < a.B;
    hrow[mb] = a.hin + (okm[mb] ? (size_t)m * a.ldhin : 0);
  }
  f32x4 acc[NRB][2];
#pragma unroll
  for (int mb = 0; mb < NRB; ++mb) { acc[mb][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[mb][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int nchunks = (D + 15) >> 4;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = wave; c < nchunks; c += 2 * GS_WAVES) {
    float4 b4[2], a4[2][NRB];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int k = (c + s * GS_WAVES) * 16 + 4 * (lane >> 4);      // D % 4 == 0: a float4 at k < D ends inside the row
      const bool okk = k < D;
      b4[s] = (okk && okb) ? *reinterpret_cast<const float4*>(wrow + k) : zero4;
#pragma unroll
      for (int mb = 0; mb < NRB; ++mb) a4[s][mb] = (okk && okm[mb]) ? *reinterpret_cast<const float4*>(hrow[mb] + k) : zero4;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float bj[4] = {b4[s].x, b4[s].y, b4[s].z, b4[s].w};
#pragma unroll
      for (int mb = 0; mb < NRB; ++mb) {
        const float aj[4] = {a4[s][mb].x, a4[s][mb].y, a4[s][mb].z, a4[s][mb].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[mb][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[j], bj[j], acc[mb][s], 0, 0, 0);
      }
    }
  }
  // C/D map of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
  for (int mb = 0; mb < NRB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][mb * 16 + (lane >> 4) * 4 + r][col] = acc[mb][0][r] + acc[mb][1][r];
  __syncthreads();
  if (tid < NRB * 16 * 4) {
    const int lr = tid >> 2, u = tid & 3;
    const int row = m0 + lr, d = u0 + u;
    if (row < a.B) {
      float gh[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < GS_WAVES; ++w) v += part[w][lr][g * 4 + u];
        gh[g] = v + a.bhh[g * D + d];
      }
      // the gate arithmetic of gru_gates_fwd_kernel (elementwise.hip)
      const float* gir = a.gi + (size_t)row * 3 * D;
      const float rg = gs_sigmoid(gir[d] + gh[0]);
      const float ug = gs_sigmoid(gir[D + d] + gh[1]);
      const float ng = tanhf(gir[2 * D + d] + rg * gh[2]);
      const float h = a.hin[(size_t)row * a.ldhin + d];
      a.hout[(size_t)row * a.ldo + d] = (h - ng) * ug + ng;
      if (a.gh_save) {      // what the backward needs: the hidden gate products (GI is kept by the batched product)
        float* s = a.gh_save + (size_t)row * 3 * D;
        s[d] = gh[0]; s[D + d] = gh[1]; s[2 * D + d] = gh[2];
      }
    }
  }
}

// y[r][:] = zero && zero[r] ? 0 : x[r][:]   (h_0 = h0 * !reset0 as a select: a reset row is exactly the zero row)
__global__ void __launch_bounds__(256) gs_copy_rows_kernel(int rows, int n, const float* __restrict__ x, int ldx,
                                                           const uint8_t* __restrict__ zero, float* __restrict__ y, int ldy) {
  const size_t total = (size_t)rows * n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int r = (int)(i / n), c = (int)(i % n);
    y[(size_t)r * ldy + c] = (zero && zero[r]) ? 0.f : x[(size_t)r * ldx + c];
  }
}
static int gs_copy_rows(int rows, int n, const float* x, int ldx, const uint8_t* zero, float* y, int ldy, hipStream_t st) {
  const size_t total = (size_t)rows * n;
  const unsigned blocks = (unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(gs_copy_rows_kernel, dim3(blocks), dim3(256), 0, st, rows, n, x, ldx, zero, y, ldy);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

static int gs_step_launch(const GruStepArgs& a, hipStream_t st) {
  // one workgroup per strip of 4 hidden units and block of 16 rows
  hipLaunchKernelGGL(gru_step_kernel, dim3(a.D / 4, dm_cdiv(a.B, 16)), dim3(GS_WAVES * 64), 0, st, a);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

static size_t gs_pad(size_t n) { return dm_align_up(n, 64); }

extern "C" size_t dm_gru_sequence_acts_floats(int T, int B, int In, int D) {
  if (T < 1 || B < 1 || In < 1 || D < 1) return 0;
  const size_t N = (size_t)T * B;
  return 2 * gs_pad(N * 3 * D) + gs_pad((size_t)B * D);
}
extern "C" size_t dm_gru_sequence_ws_bytes(int T, int B, int In, int D) {
  if (T < 1 || B < 1 || In < 1 || D < 1) return 0;
  const size_t N = (size_t)T * B;
  // split-K scratch + (forward without acts: GI, one step's GH, h_0) / (backward: dGI, dGH, two carried dh)
  return (DM_SPLITK_FLOATS + 2 * gs_pad(N * 3 * D) + 2 * gs_pad((size_t)B * D) + 64) * sizeof(float);
}

static int gs_check(const char* who, int T, int B, int In, int D, size_t ws_bytes) {
  DM_REQUIRE(T >= 1 && B >= 1 && In >= 1 && D >= 1, DM_E_SHAPE, "%s: T %d, B %d, In %d, D %d must all be >= 1", who, T, B, In, D);
  DM_REQUIRE(D % 4 == 0, DM_E_SHAPE, "%s: D %d must be a multiple of 4", who, D);
  DM_REQUIRE((int64_t)T * B * 3 * D < ((int64_t)1 << 31), DM_E_SHAPE, "%s: T*B*3D = %lld rows x columns exceed 2^31", who,
             (long long)T * B * 3 * D);
  DM_REQUIRE(ws_bytes >= dm_gru_sequence_ws_bytes(T, B, In, D), DM_E_WORKSPACE, "%s: workspace too small (%zu bytes, need %zu)", who,
             ws_bytes, dm_gru_sequence_ws_bytes(T, B, In, D));
  return DM_OK;
}

extern "C" int dm_gru_sequence_fwd(int T, int B, int In, int D, const float* x, int ldx, const float* h0, const uint8_t* reset0,
                                   const dm_gru_params* p, float* acts, float* H, int ldh, void* ws, size_t ws_bytes,
                                   void* stream) {
  DM_REQUIRE(x && h0 && p && H && ws, DM_E_NULL, "gru_sequence_fwd: null pointer");
  DM_REQUIRE(p->w_ih && p->w_hh && p->b_ih && p->b_hh, DM_E_NULL, "gru_sequence_fwd: null parameter");
  DM_TRY(gs_check("gru_sequence_fwd", T, B, In, D, ws_bytes));
  DM_REQUIRE(ldx >= In && ldh >= D, DM_E_SHAPE, "gru_sequence_fwd: ldx %d < In %d or ldh %d < D %d", ldx, In, ldh, D);
  hipStream_t st = (hipStream_t)stream;
  DmPrecisionScope prec(0);
  const size_t N = (size_t)T * B;
  DmArena wa(ws, ws_bytes);
  float* sk = wa.take(DM_SPLITK_FLOATS);
  const size_t skb = DM_SPLITK_FLOATS * sizeof(float);
  float *gi, *gh, *h0m;
  if (acts) {
    DmArena aa(acts, dm_gru_sequence_acts_floats(T, B, In, D) * sizeof(float));
    gi = aa.take(N * 3 * D); gh = aa.take(N * 3 * D); h0m = aa.take((size_t)B * D);
  } else {
    gi = wa.take(N * 3 * D); gh = wa.take((size_t)B * 3 * D); h0m = wa.take((size_t)B * D);
  }
  DM_REQUIRE(wa.ok, DM_E_WORKSPACE, "gru_sequence_fwd: workspace too small");
  // One launch per step pays where the composed pair is bound by its two launches: below the <= 64-row skinny product's floor
  // (3*D*D < 64K weights, D <= 144), where the h W_hh^T product is a single tiled workgroup.  From there up the skinny product
  // plus the gates kernel were measured 2.2 - 4.2x faster than gru_step_kernel at D 600 / 1024 / 2048.
  // (float4 loads of h_0, H and W_hh: 16-byte aligned bases and rows; h_0 is carved at a 256-byte offset of acts / ws)
  const bool aligned = (ldh & 3) == 0 && ((((uintptr_t)H | (uintptr_t)p->w_hh | (uintptr_t)h0m) & 15) == 0);
  const bool narrow = (int64_t)3 * D * D < (int64_t)64 * 1024;
  const bool fused = B <= 64 && aligned && (g_gru_fuse == 2 || (g_gru_fuse == 1 && narrow));
  tl_gru_sched = fused ? 1 : 0;

  DM_TRY(gs_copy_rows(B, D, h0, D, reset0, h0m, D, st));
  {
    DmGemm q;
    q.M = (int)N; q.N = 3 * D; q.K = In;
    q.A = x; q.lda = ldx; q.B = p->w_ih; q.ldb = In; q.C = gi; q.ldc = 3 * D; q.bias = p->b_ih;
    DM_TRY(dm_gemm_launch(q, sk, skb, st));
  }
  for (int t = 0; t < T; ++t) {
    const float* hin = t == 0 ? h0m : H + (size_t)(t - 1) * B * ldh;
    const int ldhin = t == 0 ? D : ldh;
    float* hout = H + (size_t)t * B * ldh;
    const float* gi_t = gi + (size_t)t * B * 3 * D;
    float* gh_t = acts ? gh + (size_t)t * B * 3 * D : gh;
    if (fused) {
      GruStepArgs a;
      a.whh = p->w_hh; a.bhh = p->b_hh; a.gi = gi_t; a.hin = hin; a.ldhin = ldhin; a.hout = hout; a.ldo = ldh;
      a.gh_save = acts ? gh_t : nullptr; a.B = B; a.D = D;
      DM_TRY(gs_step_launch(a, st));
    } else {
      DmGemm q;
      q.M = B; q.N = 3 * D; q.K = D;
      q.A = hin; q.lda = ldhin; q.B = p->w_hh; q.ldb = D; q.C = gh_t; q.ldc = 3 * D; q.bias = p->b_hh;
      DM_TRY(dm_gemm_launch(q, sk, skb, st));
      DM_TRY(dm_gru_gates_fwd_launch(B, D, gi_t, gh_t, hin, ldhin, hout, ldh, nullptr, nullptr, nullptr, nullptr, st));
    }
  }
  return DM_OK;
}

extern "C" int dm_gru_sequence_bwd(int T, int B, int In, int D, const float* x, int ldx, const dm_gru_params* p, const float* acts,
                                   const float* H, int ldh, const float* dH, int lddh, const dm_gru_grads* g, float* dx, int lddx,
                                   void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(x && p && acts && H && dH && g && ws, DM_E_NULL, "gru_sequence_bwd: null pointer");
  DM_REQUIRE(p->w_ih && p->w_hh && p->b_ih && p->b_hh, DM_E_NULL, "gru_sequence_bwd: null parameter");
  DM_REQUIRE(g->w_ih && g->w_hh && g->b_ih && g->b_hh, DM_E_NULL, "gru_sequence_bwd: null gradient buffer");
  DM_TRY(gs_check("gru_sequence_bwd", T, B, In, D, ws_bytes));
  DM_REQUIRE(ldx >= In && ldh >= D && lddh >= D && (!dx || lddx >= In), DM_E_SHAPE,
             "gru_sequence_bwd: leading dimension too small (ldx %d, ldh %d, lddh %d, lddx %d)", ldx, ldh, lddh, lddx);
  hipStream_t st = (hipStream_t)stream;
  DmPrecisionScope prec(0);
  const size_t N = (size_t)T * B;
  DmArena aa(const_cast<float*>(acts), dm_gru_sequence_acts_floats(T, B, In, D) * sizeof(float));
  const float* gi = aa.take(N * 3 * D);
  const float* gh = aa.take(N * 3 * D);
  const float* h0m = aa.take((size_t)B * D);
  DmArena wa(ws, ws_bytes);
  float* sk = wa.take(DM_SPLITK_FLOATS);
  const size_t skb = DM_SPLITK_FLOATS * sizeof(float);
  float* dgi = wa.take(N * 3 * D);
  float* dgh = wa.take(N * 3 * D);
  float* cur = wa.take((size_t)B * D);
  float* nxt = wa.take((size_t)B * D);
  DM_REQUIRE(wa.ok, DM_E_WORKSPACE, "gru_sequence_bwd: workspace too small");

  // the BPTT loop: cur = dL/dh_t complete (dH_t + what flows back from step t + 1)
  DM_TRY(gs_copy_rows(B, D, dH + (size_t)(T - 1) * B * lddh, lddh, nullptr, cur, D, st));
  for (int t = T - 1; t >= 0; --t) {
    const size_t r0 = (size_t)t * B;
    const float* hin = t == 0 ? h0m : H + (size_t)(t - 1) * B * ldh;
    const int ldhin = t == 0 ? D : ldh;
    // no gradient goes to h0: step 0 writes only its gate gradients
    DM_TRY(dm_gru_gates_bwd_launch(B, D, gi + r0 * 3 * D, gh + r0 * 3 * D, hin, ldhin, cur, D, dgi + r0 * 3 * D, dgh + r0 * 3 * D,
                                   t > 0 ? nxt : nullptr, D, 0, nullptr, st));
    if (t > 0) {      // nxt = dh_t z (above) + dGH_t W_hh + dH_{t-1}
      DmGemm q;
      q.a_layout = 0; q.b_layout = 1;
      q.M = B; q.N = D; q.K = 3 * D;
      q.A = dgh + r0 * 3 * D; q.lda = 3 * D; q.B = p->w_hh; q.ldb = D; q.C = nxt; q.ldc = D;
      q.add = dH + (size_t)(t - 1) * B * lddh; q.ldadd = lddh;
      q.flags = DM_GEMM_ACCUM;
      DM_TRY(dm_gemm_launch(q, sk, skb, st));
      float* tmp = cur; cur = nxt; nxt = tmp;
    }
  }
  // parameter gradients over all T*B rows (overwritten), then dX
  {
    DmGemm q;      // dW_ih = dGI^T X
    q.a_layout = 1; q.b_layout = 1;
    q.M = 3 * D; q.N = In; q.K = (int)N;
    q.A = dgi; q.lda = 3 * D; q.B = x; q.ldb = ldx; q.C = g->w_ih; q.ldc = In;
    DM_TRY(dm_gemm_launch(q, sk, skb, st));
  }
  {
    DmGemm q;      // dW_hh = dGH^T [h_0; H_0 .. H_{T-2}]: the h_0 rows first, the rows of H accumulated behind them
    q.a_layout = 1; q.b_layout = 1;
    q.M = 3 * D; q.N = D; q.K = B;
    q.A = dgh; q.lda = 3 * D; q.B = h0m; q.ldb = D; q.C = g->w_hh; q.ldc = D;
    DM_TRY(dm_gemm_launch(q, sk, skb, st));
    if (T > 1) {
      q.K = (int)(N - B);
      q.A = dgh + (size_t)B * 3 * D; q.B = H; q.ldb = ldh;
      q.flags = DM_GEMM_ACCUM;
      DM_TRY(dm_gemm_launch(q, sk, skb, st));
    }
  }
  DM_TRY(dm_colsum_launch((int)N, 3 * D, dgi, 3 * D, g->b_ih, sk, skb, st));
  DM_TRY(dm_colsum_launch((int)N, 3 * D, dgh, 3 * D, g->b_hh, sk, skb, st));
  if (dx) {
    DmGemm q;      // dX = dGI W_ih
    q.a_layout = 0; q.b_layout = 1;
    q.M = (int)N; q.N = In; q.K = 3 * D;
    q.A = dgi; q.lda = 3 * D; q.B = p->w_ih; q.ldb = In; q.C = dx; q.ldc = lddx;
    DM_TRY(dm_gemm_launch(q, sk, skb, st));
  }
  return DM_OK;
}
