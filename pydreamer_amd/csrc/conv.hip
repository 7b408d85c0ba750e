// ConvEncoder (encoders.py:72-96) and ConvDecoder + MSE (decoders.py:111-180) as GEMMs over stride-2 patch
// matrices.  Internal activations are NHWC so that a patch row (ky,kx,c) is contiguous in c and every
// gather/scatter kernel below moves 16-byte vectors; weights are re-laid once per call from the torch
// layouts (O,I,kh,kw) / (I,O,kh,kw) to (O,kh,kw,I) / (I,kh,kw,O) and gradients are permuted back.
//
//   conv   k4 s2 : Y[(n,ys,xs)][o]          = ELU( im2col(X)[(n,ys,xs)][(ky,kx,i)] . Wr[o][(ky,kx,i)] + b[o] )
//   convT  k  s2 : Ycol[(n,ys,xs)][(ky,kx,o)] = X[(n,ys,xs)][i] . Wr[i][(ky,kx,o)] ;  out = col2im(Ycol) + b (+ELU)
// The backward passes are the same two gathers with the roles swapped (convT backward-data is a conv).
// All kernels here are HBM-streaming; the contractions run in gemm.hip on the matrix cores.
#include "common.h"
#include <algorithm>

// ---------------------------------------------------------------- patch gather ------------------
// col[(i,ys,xs)][(ky,kx,cc)] = big[i, 2ys+ky, 2xs+kx, cc]      (NHWC, VEC floats of c per thread)
template <int VEC>
__global__ void __launch_bounds__(256) im2col_s2_nhwc_kernel(int n, int hb, int wb, int c, int k, int hs, int ws,
                                                             const float* __restrict__ big, float* __restrict__ col) {
  const int cv = c / VEC;
  const size_t total = (size_t)n * hs * ws * k * k * cv;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int c4 = (int)(t % cv); t /= cv;
    const int kx = (int)(t % k); t /= k;
    const int ky = (int)(t % k); t /= k;
    const int xs = (int)(t % ws); t /= ws;
    const int ys = (int)(t % hs); t /= hs;
    const int i = (int)t;
    const size_t src = (((size_t)i * hb + (2 * ys + ky)) * wb + (2 * xs + kx)) * c + (size_t)c4 * VEC;
    if constexpr (VEC == 4) {
      reinterpret_cast<float4*>(col)[e] = *reinterpret_cast<const float4*>(big + src);
    } else {
      col[e] = big[src];
    }
  }
}

// layer-1 variant reading the (T,B,C,H,W) batch directly: col[(i,ys,xs)][(cc,ky,kx)] = big[i, cc, 2ys+ky, 2xs+kx]
__global__ void __launch_bounds__(256) im2col_s2_nchw_kernel(int n, int hb, int wb, int c, int k, int hs, int ws,
                                                             const float* __restrict__ big, float* __restrict__ col) {
  const size_t total = (size_t)n * hs * ws * c * k * k;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int kx = (int)(t % k); t /= k;
    const int ky = (int)(t % k); t /= k;
    const int cc = (int)(t % c); t /= c;
    const int xs = (int)(t % ws); t /= ws;
    const int ys = (int)(t % hs); t /= hs;
    const int i = (int)t;
    col[e] = big[(((size_t)i * c + cc) * hb + (2 * ys + ky)) * wb + (2 * xs + kx)];
  }
}

// the same patch matrix straight from the replay's native uint8 (T,B,H,W,C) frames (preprocessing.py:21-29 `to_image`:
// x/255 - 0.5 and HWC -> CHW happen HERE, in the first conv's patch loader - SURVEY 8(f) N1): the float image is never
// materialised, the frames cross HBM as 1 byte per element.  col[(i,ys,xs)][(cc,ky,kx)] = u8[i, 2ys+ky, 2xs+kx, cc]/255 - 0.5
__global__ void __launch_bounds__(256) im2col_s2_u8hwc_kernel(int n, int hb, int wb, int c, int k, int hs, int ws,
                                                              const uint8_t* __restrict__ big, float* __restrict__ col) {
  const size_t total = (size_t)n * hs * ws * c * k * k;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int kx = (int)(t % k); t /= k;
    const int ky = (int)(t % k); t /= k;
    const int cc = (int)(t % c); t /= c;
    const int xs = (int)(t % ws); t /= ws;
    const int ys = (int)(t % hs); t /= hs;
    const int i = (int)t;
    col[e] = (float)big[(((size_t)i * hb + (2 * ys + ky)) * wb + (2 * xs + kx)) * c + cc] / 255.0f - 0.5f;
  }
}

// big[i,y,x,cc] = epi( bias[cc] + sum_{ky,kx : (y-ky),(x-kx) even, in range} col[(i,(y-ky)/2,(x-kx)/2)][(ky,kx,cc)] )
template <int VEC>
__global__ void __launch_bounds__(256) col2im_s2_kernel(int n, int hb, int wb, int c, int k, int hs, int ws,
                                                        const float* __restrict__ col, const float* __restrict__ bias,
                                                        int flags, const float* __restrict__ elu_ref,
                                                        float* __restrict__ big, unsigned short* __restrict__ big_h) {
  const int cv = c / VEC;
  const size_t total = (size_t)n * hb * wb * cv;
  const size_t rowlen = (size_t)k * k * c;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int c4 = (int)(t % cv); t /= cv;
    const int x = (int)(t % wb); t /= wb;
    const int y = (int)(t % hb); t /= hb;
    const int i = (int)t;
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = bias ? bias[c4 * VEC + q] : 0.f;
    for (int ky = y & 1; ky < k && ky <= y; ky += 2) {
      const int ys = (y - ky) >> 1;
      if (ys >= hs) continue;
      for (int kx = x & 1; kx < k && kx <= x; kx += 2) {
        const int xs = (x - kx) >> 1;
        if (xs >= ws) continue;
        const float* p = col + (((size_t)i * hs + ys) * ws + xs) * rowlen + (size_t)(ky * k + kx) * c + (size_t)c4 * VEC;
        if constexpr (VEC == 4) {
          const float4 v = *reinterpret_cast<const float4*>(p);
          acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
        } else {
          acc[0] += p[0];
        }
      }
    }
    const size_t dst = e * VEC;
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      float v = acc[q];
      if (flags & DM_C2I_ELU) v = dm_elu(v);
      if (elu_ref) v *= dm_elu_grad_from_y(elu_ref[dst + q]);
      big[dst + q] = v;
      if (big_h) big_h[dst + q] = (unsigned short)dm_f2bf(v);
    }
  }
}

static inline int grid_for(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

int dm_im2col_s2_launch(int n, int hb, int wb, int c, int k, const float* big, int big_nchw, float* col, hipStream_t st) {
  // "valid" stride-2 geometry: a trailing row/column that no window reaches is simply never read (31 -> 14 at k=4)
  DM_REQUIRE(hb >= k && wb >= k && k >= 1, DM_E_SHAPE, "im2col_s2: big %dx%d smaller than k=%d", hb, wb, k);
  const int hs = (hb - k) / 2 + 1, ws = (wb - k) / 2 + 1;
  const size_t total = (size_t)n * hs * ws * k * k * c;
  if (total == 0) return DM_OK;
  if (big_nchw) {
    hipLaunchKernelGGL(im2col_s2_nchw_kernel, dim3(grid_for(total)), dim3(256), 0, st, n, hb, wb, c, k, hs, ws, big, col);
  } else if ((c & 3) == 0 && (((uintptr_t)big | (uintptr_t)col) & 15) == 0) {
    hipLaunchKernelGGL((im2col_s2_nhwc_kernel<4>), dim3(grid_for(total / 4)), dim3(256), 0, st, n, hb, wb, c, k, hs, ws,
                       big, col);
  } else {
    hipLaunchKernelGGL((im2col_s2_nhwc_kernel<1>), dim3(grid_for(total)), dim3(256), 0, st, n, hb, wb, c, k, hs, ws, big,
                       col);
  }
  DM_LAUNCH_CHECK();
  return DM_OK;
}

int dm_col2im_s2_launch(int n, int hb, int wb, int c, int k, const float* col, const float* bias, int flags,
                        const float* elu_ref, float* big, hipStream_t st) {
  // rows/columns of `big` that no window reaches receive only the bias (zero gradient in the conv backward use)
  DM_REQUIRE(hb >= k && wb >= k && k >= 1, DM_E_SHAPE, "col2im_s2: big %dx%d smaller than k=%d", hb, wb, k);
  const int hs = (hb - k) / 2 + 1, ws = (wb - k) / 2 + 1;
  const size_t total = (size_t)n * hb * wb * c;
  if (total == 0) return DM_OK;
  unsigned short* big_h = dm_twin_of(big, false);      // bf16 mode: the result's twin (common.h DmTwinScope), written here
  if (big_h) dm_twin_mark(big);
  if ((c & 3) == 0 && (((uintptr_t)big | (uintptr_t)col) & 15) == 0) {
    hipLaunchKernelGGL((col2im_s2_kernel<4>), dim3(grid_for(total / 4)), dim3(256), 0, st, n, hb, wb, c, k, hs, ws, col,
                       bias, flags, elu_ref, big, big_h);
  } else {
    hipLaunchKernelGGL((col2im_s2_kernel<1>), dim3(grid_for(total)), dim3(256), 0, st, n, hb, wb, c, k, hs, ws, col, bias,
                       flags, elu_ref, big, big_h);
  }
  DM_LAUNCH_CHECK();
  return DM_OK;
}

extern "C" int dm_im2col_s2(int n, int hb, int wb, int c, int k, const float* big, int big_nchw, float* col, void* stream) {
  DM_REQUIRE(big && col, DM_E_NULL, "im2col_s2: null pointer");
  return dm_im2col_s2_launch(n, hb, wb, c, k, big, big_nchw, col, (hipStream_t)stream);
}
extern "C" int dm_col2im_s2(int n, int hb, int wb, int c, int k, const float* col, const float* bias, int flags,
                            const float* elu_ref, float* big, void* stream) {
  DM_REQUIRE(big && col, DM_E_NULL, "col2im_s2: null pointer");
  return dm_col2im_s2_launch(n, hb, wb, c, k, col, bias, flags, elu_ref, big, (hipStream_t)stream);
}

// dst[j0,j1,j2,j3] = src[i0,i1,i2,i3] with j_a = i_{p_a}  (dst dims = (d[p0],d[p1],d[p2],d[p3]))
__global__ void __launch_bounds__(256) permute4_kernel(const float* __restrict__ src, float* __restrict__ dst, int d0,
                                                       int d1, int d2, int d3, int p0, int p1, int p2, int p3) {
  const int d[4] = {d0, d1, d2, d3};
  const int p[4] = {p0, p1, p2, p3};
  const size_t total = (size_t)d0 * d1 * d2 * d3;
  const size_t sstride[4] = {(size_t)d1 * d2 * d3, (size_t)d2 * d3, (size_t)d3, 1};
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    size_t s = 0;
#pragma unroll
    for (int a = 3; a >= 0; --a) {
      const int dim = d[p[a]];
      const int j = (int)(t % dim);
      t /= dim;
      s += (size_t)j * sstride[p[a]];
    }
    dst[e] = src[s];
  }
}
int dm_permute4_launch(const float* src, float* dst, int d0, int d1, int d2, int d3, int p0, int p1, int p2, int p3,
                       hipStream_t st) {
  const size_t total = (size_t)d0 * d1 * d2 * d3;
  if (total == 0) return DM_OK;
  hipLaunchKernelGGL(permute4_kernel, dim3(grid_for(total)), dim3(256), 0, st, src, dst, d0, d1, d2, d3, p0, p1, p2, p3);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

// ---------------------------------------------------------------- implicit im2col tables ----------
// The stride-2 patch matrix col[(i,ys,xs)][(ky,kx,c)] = big[i, 2ys+ky, 2xs+kx, c] (NHWC) is a SEPARABLE gather:
//   address = rowoff[(i,ys,xs)] + koff[(ky,kx,c)],  rowoff = ((i*hb + 2ys)*wb + 2xs)*c,  koff = ky*wb*c + kx*c + cc
// so the GEMM loaders (gemm.hip, gather operands) read patches straight from the activation tensor and the patch
// matrix is never materialised.  Both tables are tiny (rows + k*k*c ints) and L2-resident.
__global__ void __launch_bounds__(256) conv_tables_kernel(int n, int hb, int wb, int c, int k, int hs, int ws,
                                                          int* __restrict__ rowoff, int* __restrict__ koff) {
  const int rows = n * hs * ws;
  const int kc = k * c;
  const int kdim = k * kc;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < rows + kdim; e += gridDim.x * 256) {
    if (e < rows) {
      const int xs = e % ws, ys = (e / ws) % hs, i = e / (ws * hs);
      rowoff[e] = ((i * hb + 2 * ys) * wb + 2 * xs) * c;
    } else {
      const int q = e - rows;
      koff[q] = (q / kc) * (wb * c) + q % kc;
    }
  }
}
static int conv_tables_launch(int n, int hb, int wb, int c, int k, int* rowoff, int* koff, hipStream_t st) {
  const int hs = (hb - k) / 2 + 1, ws = (wb - k) / 2 + 1;
  DM_REQUIRE((int64_t)n * hb * wb * c < ((int64_t)1 << 31), DM_E_SHAPE, "conv tables: tensor exceeds 2^31 elements");
  const int total = n * hs * ws + k * k * c;
  hipLaunchKernelGGL(conv_tables_kernel, dim3(grid_for(total)), dim3(256), 0, st, n, hb, wb, c, k, hs, ws, rowoff, koff);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

// ---------------------------------------------------------------- gather-form transposed convolution ----------
// ConvTranspose2d(k even, stride 2) WITHOUT a column matrix (decoders.py:144-161; the same identity gives the data
// gradient of a stride-2 Conv2d).  out[n, 2yy+py, 2xx+px, o] = b[o] + sum_{a,b,i} X[n, yy-a, xx-b, i] W[i][o][py+2a][px+2b]
// with a, b in [0, k/2): every parity class (py,px) reads the SAME input patch, so the layer is ONE GEMM
//   M = n*Hc*Wc class pixels (Hc = hs + k/2 - 1),  K = (k/2)^2 * cin (gathered from a zero-padded copy of X),
//   N = 4*cout (the four classes side by side), result scattered straight into the NHWC big image (gemm.hip SC epilogue).
// vs. the column-matrix form: no Ycol write + col2im read (2 x 2.9 GB for decoder layer 3 at Atari-literal), at the price
// of (Hc/hs)^2 more MACs where the zero border is multiplied too (1.33x for 13 -> 30).
// Not multiplying it (fp32 products, dm_convt_kskip_enable): a class pixel (yy, xx) has tap (a, b) inside the input iff
// 0 <= yy-a < hs and 0 <= xx-b < ws - between one and k/2 taps per dimension - and the reduction index is (a, b, i), so an
// invalid tap is a run of cin zeros in the patch.  Rows are therefore enumerated frame-chunk-major, (chunk of CONVT_G frames,
// yy, xx, frame in chunk): a 64- or 128-row tile of the product then lies inside ONE class pixel, consecutive tiles walk
// neighbouring pixels of the same frames (their overlapping patches meet in L2), and the table launch writes, per block of
// CONVT_G rows, the ascending list of the 32-k tiles that hold at least one tap valid for some row of the block
// (DmGemm::k_list).  The tile loops walk that list instead of every tile.  The terms left out are 0 * w and the terms kept are
// added in the same order, so the result has the same bits for every finite weight (a non-finite weight would turn 0 * w into
// NaN; such a run is broken already, the border contributes nothing by definition, and the skipped form is the right one).
// The zero-padded copy stays: a kept tile may still hold invalid taps (cin not a multiple of 32, the short last chunk whose
// blocks straddle pixels), so the list only has to be a superset and correctness never depends on its being tight.
constexpr int CONVT_G = 128;
static int g_convt_kskip = 1;
// 1 / 0: the chunk-major row order with k-tile lists / the (frame, yy, xx) order with every tile, -1: query.  Returns the state.
extern "C" int dm_convt_kskip_enable(int on) {
  if (on >= 0) g_convt_kskip = on ? 1 : 0;
  return g_convt_kskip;
}
static inline size_t convt_klist_ints(size_t rows, int kdim) { return (size_t)dm_cdiv((int64_t)rows, CONVT_G) * (dm_cdiv(kdim, 32) + 1); }
__global__ void __launch_bounds__(256) convt_pad_kernel(int n, int hs, int ws, int c4, int P, const float4* __restrict__ x,
                                                        float4* __restrict__ xp) {
  const int hp = hs + 2 * P, wp = ws + 2 * P;
  const size_t total = (size_t)n * hp * wp * c4;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int cc = (int)(t % c4); t /= c4;
    const int xx = (int)(t % wp) - P; t /= wp;
    const int yy = (int)(t % hp) - P; t /= hp;
    const int i = (int)t;
    const bool in = yy >= 0 && yy < hs && xx >= 0 && xx < ws;
    xp[e] = in ? x[(((size_t)i * hs + yy) * ws + xx) * c4 + cc] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// The same zero-padded copy written as bf16 (the gathered operand of a bf16-storage product, common.h DmTwinScope)
__global__ void __launch_bounds__(256) convt_pad_h_kernel(int n, int hs, int ws, int c4, int P, const float4* __restrict__ x,
                                                          uint2* __restrict__ xp) {
  const int hp = hs + 2 * P, wp = ws + 2 * P;
  const size_t total = (size_t)n * hp * wp * c4;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int cc = (int)(t % c4); t /= c4;
    const int xx = (int)(t % wp) - P; t /= wp;
    const int yy = (int)(t % hp) - P; t /= hp;
    const int i = (int)t;
    const bool in = yy >= 0 && yy < hs && xx >= 0 && xx < ws;
    xp[e] = in ? dm_pack_bf16x4(x[(((size_t)i * hs + yy) * ws + xx) * c4 + cc]) : make_uint2(0u, 0u);
  }
}
// rowoff[(n,yy,xx)] = offset of padded pixel (yy+P, xx+P);  koff[(a,b,i)] = -(a*wp + b)*cin + i;
// ctab[(n,yy,xx)] = {offset of big[n, 2yy, 2xx, 0], bit 1: 2yy+1 < hb, bit 0: 2xx+1 < wb}
// Row e of the product: G == 0: (frame, yy, xx); G > 0: (chunk of G frames, yy, xx, frame in chunk), the last chunk possibly
// short (no padded rows).  Both tables are indexed by e, and they are all the product knows about its rows.
__device__ __forceinline__ void convt_row_of(int e, int n, int Hc, int Wc, int G, int* i, int* pix) {
  if (G == 0) { *i = e / (Wc * Hc); *pix = e - *i * (Wc * Hc); return; }
  const int per = G * Hc * Wc;
  const int c = e / per, r = e - c * per;
  const int gl = min(G, n - c * G);
  *pix = r / gl;
  *i = c * G + (r - *pix * gl);
}
// klist (G > 0): for block j of G rows, klist[j * (nkt + 1)] = count and then the ascending indices of the 32-k tiles that hold a
// tap (a, b) with 0 <= yy-a < hs and 0 <= xx-b < ws for some row of the block.  A block lies inside one chunk (a full chunk is
// a multiple of G rows), so its rows are a run of pixels in raster order: the rows yy0..yy1 and, when the run stays in one
// pixel row, the columns xx0..xx1 (all columns otherwise) bound the valid taps per dimension - a superset, tight when the
// block is one pixel.
__global__ void __launch_bounds__(256) convt_tables_kernel(int n, int hs, int ws, int cin, int ta, int hb, int wb, int cout,
                                                           int* __restrict__ rowoff, int* __restrict__ koff,
                                                           int2* __restrict__ ctab, int G, int* __restrict__ klist) {
  const int P = ta - 1, hp = hs + 2 * P, wp = ws + 2 * P;
  const int Hc = hs + ta - 1, Wc = ws + ta - 1;
  const int rows = n * Hc * Wc, kdim = ta * ta * cin;
  const int nkt = (kdim + 31) / 32, nblk = G > 0 ? (rows + G - 1) / G : 0;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < rows + kdim + nblk; e += gridDim.x * 256) {
    if (e < rows) {
      int i, pix;
      convt_row_of(e, n, Hc, Wc, G, &i, &pix);
      const int xx = pix % Wc, yy = pix / Wc;
      rowoff[e] = ((i * hp + yy + P) * wp + xx + P) * cin;
      ctab[e] = make_int2(((i * hb + 2 * yy) * wb + 2 * xx) * cout, ((2 * yy + 1 < hb) ? 2 : 0) | ((2 * xx + 1 < wb) ? 1 : 0));
    } else if (e < rows + kdim) {
      const int q = e - rows;
      const int ci = q % cin, b = (q / cin) % ta, a = q / (cin * ta);
      koff[q] = -(a * wp + b) * cin + ci;
    } else {
      const int j = e - rows - kdim;
      int i0, p0, i1, p1;
      convt_row_of(j * G, n, Hc, Wc, G, &i0, &p0);
      convt_row_of(min(rows, (j + 1) * G) - 1, n, Hc, Wc, G, &i1, &p1);
      const int y0 = p0 / Wc, y1 = p1 / Wc;
      const int x0 = y0 == y1 ? p0 % Wc : 0, x1 = y0 == y1 ? p1 % Wc : Wc - 1;
      int* kl = klist + (size_t)j * (nkt + 1);
      int cnt = 0;
      for (int t = 0; t < nkt; ++t) {
        const int q0 = (32 * t) / cin, q1 = min(32 * t + 31, kdim - 1) / cin;
        bool keep = false;
        for (int q = q0; q <= q1; ++q) {
          const int a = q / ta, b = q % ta;
          keep = keep || (a <= y1 && y0 <= hs - 1 + a && b <= x1 && x0 <= ws - 1 + b);
        }
        if (keep) kl[1 + cnt++] = t;
      }
      kl[0] = cnt;
    }
  }
}
// One launch of the tables (and, with klist, of the chunk-major order and the k-tile lists)
static int convt_tables_launch(int n, int hs, int cin, int ta, int hb, int cout, int* rowoff, int* koff, int2* ctab, int* klist,
                               hipStream_t st) {
  const int Hc = hs + ta - 1, kdim = ta * ta * cin;
  const size_t total = (size_t)n * Hc * Hc + kdim + (klist ? (size_t)dm_cdiv((int64_t)n * Hc * Hc, CONVT_G) : 0);
  hipLaunchKernelGGL(convt_tables_kernel, dim3(grid_for(total)), dim3(256), 0, st, n, hs, hs, cin, ta, hb, hb, cout, rowoff, koff,
                     ctab, klist ? CONVT_G : 0, klist);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
// Wcat[(py,px,o)][(a,b,i)] = W[i][o][py+2a][px+2b]      (W: torch ConvTranspose2d layout (cin, cout, k, k))
__global__ void __launch_bounds__(256) convt_repack_kernel(int cin, int cout, int k, const float* __restrict__ w,
                                                           float* __restrict__ wcat) {
  const int ta = k / 2, kdim = ta * ta * cin;
  const int total = 4 * cout * kdim;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int kk = e % kdim, nn = e / kdim;
    const int ci = kk % cin, b = (kk / cin) % ta, a = kk / (cin * ta);
    const int o = nn % cout, cls = nn / cout, py = cls >> 1, px = cls & 1;
    wcat[e] = w[(((size_t)ci * cout + o) * k + (py + 2 * a)) * k + (px + 2 * b)];
  }
}
// The big image of a scatter product whose extent hb is odd (encoder layer 1's 31 x 31 output under the layer-2 data gradient):
// the class grid covers rows / columns 0 .. E-1 with E = 2*Hc = hb - 1 and the epilogue writes every one of those (each class
// pixel has its four parities inside, c_tab's two range bits all set; M and N of the product are exact), so only the rows and
// columns E .. hb-1, which no window reaches, have to be cleared: (hb^2 - E^2) pixels per frame instead of the whole buffer
// (29 MB of 461 MB at Atari-literal).  V channels per thread (4: 16-byte stores); out_h: optional bf16 twin.
template <int V>
__global__ void __launch_bounds__(256) convt_border_zero_kernel(int n, int hb, int E, int cv, float* __restrict__ out,
                                                                unsigned short* __restrict__ out_h) {
  const int side = hb - E, nb = hb * hb - E * E;      // border pixels of a frame: E rows of `side`, then hb - E whole rows
  const size_t total = (size_t)n * nb * cv;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    size_t t = e;
    const int cc = (int)(t % cv); t /= cv;
    const int j = (int)(t % nb);
    const int i = (int)(t / nb);
    const int y = j < E * side ? j / side : E + (j - E * side) / hb;
    const int x = j < E * side ? E + j % side : (j - E * side) % hb;
    const size_t at = ((((size_t)i * hb + y) * hb + x) * cv + cc) * V;
    if (V == 4) {
      *reinterpret_cast<float4*>(out + at) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (out_h) *reinterpret_cast<uint2*>(out_h + at) = make_uint2(0u, 0u);
    } else {
      out[at] = 0.f;
      if (out_h) out_h[at] = 0;
    }
  }
}
// layers this form is used for: even kernel, 16-byte gathers, and enough output channels that N = 4*cout fills MFMA tiles
// (and an input large enough that the zero border stays under 40 % extra MACs: (Hc/hs)^2 <= 1.4, i.e. hs >= 6 for k = 4 and
// hs >= 11 for k = 6.  The fp32 products skip the border's k-tiles - see above - wherever a tap is a whole number of tiles;
// the bound is kept as it is: admitting more layers changes which form, and so which summation order, a layer takes)
static bool convt_gather_ok(int k, int cin, int cout, int hs, size_t n) {
  const int Hc = hs + k / 2 - 1;
  return (k & 1) == 0 && (cin & 3) == 0 && cout >= 16 && 10 * Hc * Hc <= 14 * hs * hs &&
         n * (size_t)(2 * (hs - 1) + k + 1) * (2 * (hs - 1) + k + 1) * cout < ((size_t)1 << 31);
}
// What one such layer needs beside its operands: floats of the zero-padded input copy, rows of the gather / scatter tables, floats of
// the class-concatenated weights, ints of the k-tile lists; zeros and ok = false where the form is refused.  An operator folds its layers.
struct ConvtScratch {
  bool ok = false; size_t pad = 0, tab = 0, wcat = 0, klist = 0;
  void fold(const ConvtScratch& s) {
    ok |= s.ok; pad = std::max(pad, s.pad); tab = std::max(tab, s.tab); wcat = std::max(wcat, s.wcat); klist = std::max(klist, s.klist);
  }
};
static ConvtScratch convt_gather_scratch(int k, int cin, int cout, int hs, size_t n) {
  ConvtScratch s;
  if (!(s.ok = convt_gather_ok(k, cin, cout, hs, n))) return s;
  const size_t ta = k / 2, kdim = ta * ta * cin, hp = hs + 2 * (ta - 1), Hc = hs + ta - 1;
  s.pad = n * hp * hp * cin; s.tab = n * Hc * Hc; s.wcat = (size_t)4 * cout * kdim; s.klist = convt_klist_ints(s.tab, kdim);
  return s;
}
// The scratch block itself, carved the same way by every operator that has such layers.  koff_cap: ints of the k offset table
// (it is indexed by (a, b, i): (k/2)^2 * cin of the widest layer the operator admits).  wcat_h: bf16 copy of wcat (bf16 mode).
struct ConvtWs {
  float *pad, *wcat; unsigned short* wcat_h;
  int *t_rowoff, *t_koff, *t_klist; int2* t_ctab; int koff_cap;
};
static void convt_gather_carve(DmArena& ar, const ConvtScratch& s, int koff_cap, bool tw_on, ConvtWs* w) {
  w->pad = ar.take(s.pad);
  w->t_rowoff = (int*)ar.take(s.tab);
  w->t_ctab = (int2*)ar.take(2 * s.tab);
  w->t_koff = (int*)ar.take(w->koff_cap = s.wcat ? koff_cap : 0);
  w->wcat = ar.take(s.wcat);
  w->wcat_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(s.wcat) : 0);
  w->t_klist = (int*)ar.take(s.klist);      // (sized whether or not dm_convt_kskip_enable is on)
}
// One layer: a (cin -> cout) ConvTranspose2d(k, stride 2) from n x hs x hs x cin (src, NHWC) to n x hb x hb x cout (dst, NHWC),
// w in the torch layout (cin, cout, k, k).  dst = act(bias + ...) * ELU'(mulref).  hb = 2 (hs + k/2 - 1) for a transposed
// convolution proper; the data gradient of a stride-2 convolution over an odd extent has one more row / column, cleared here.
struct ConvtGather {
  const char* what; int n, hs, hb, k, cin, cout;
  const float *src, *w; float* dst;
  const float *bias = nullptr, *mulref = nullptr; int flags = 0; bool no_twin = false;
};
// hpath: the padded copy and the weights are stored as bf16 (the product reads those); klist_on: chunk-major rows and k-tile lists
static int convt_gather_launch(const ConvtGather& c, const ConvtWs& w, bool hpath, bool klist_on, float* splitk, hipStream_t st) {
  const int ta = c.k / 2, Hc = c.hs + ta - 1, hp = c.hs + 2 * (ta - 1), kdim = ta * ta * c.cin;
  DM_REQUIRE(kdim <= w.koff_cap, DM_E_SHAPE, "%s: gather-form K %d exceeds the offset table", c.what, kdim);
  const size_t padn = (size_t)c.n * hp * hp * (c.cin / 4);
  if (hpath) hipLaunchKernelGGL(convt_pad_h_kernel, dim3(grid_for(padn)), dim3(256), 0, st, c.n, c.hs, c.hs, c.cin / 4, ta - 1,
                                (const float4*)c.src, (uint2*)w.pad);
  else hipLaunchKernelGGL(convt_pad_kernel, dim3(grid_for(padn)), dim3(256), 0, st, c.n, c.hs, c.hs, c.cin / 4, ta - 1,
                          (const float4*)c.src, (float4*)w.pad);
  DM_LAUNCH_CHECK();
  int* klist = klist_on ? w.t_klist : nullptr;
  DM_TRY(convt_tables_launch(c.n, c.hs, c.cin, ta, c.hb, c.cout, w.t_rowoff, w.t_koff, w.t_ctab, klist, st));
  hipLaunchKernelGGL(convt_repack_kernel, dim3(grid_for((size_t)4 * c.cout * kdim)), dim3(256), 0, st, c.cin, c.cout, c.k, c.w,
                     w.wcat);
  DM_LAUNCH_CHECK();
  const DmCvtSeg sg = {w.wcat, w.wcat_h, (size_t)4 * c.cout * kdim};
  if (hpath) DM_TRY(dm_to_bf16_multi_launch(&sg, 1, st));
  if (2 * Hc != c.hb) {      // odd extent (31): the last row / column is reached by no window; the scatter epilogue writes the rest
    const int E = 2 * Hc, nb = c.hb * c.hb - E * E, V = (c.cout & 3) == 0 ? 4 : 1;
    hipLaunchKernelGGL(V == 4 ? convt_border_zero_kernel<4> : convt_border_zero_kernel<1>, dim3(grid_for((size_t)c.n * nb * (c.cout / V))),
                       dim3(256), 0, st, c.n, c.hb, E, c.cout / V, c.dst, dm_twin_of(c.dst, false));
    DM_LAUNCH_CHECK();
  }
  DmGemm q;   // big[n, 2yy+py, 2xx+px, o] = act( b[o] + patch(n,yy,xx) . Wcat[(py,px,o)] ) * ELU'(mulref)
  q.M = c.n * Hc * Hc; q.N = 4 * c.cout; q.K = kdim;
  q.A = w.pad; q.a_maj = w.t_rowoff; q.a_min = w.t_koff; q.a_tab_vec = 1; q.a_tab_vec8 = 1;
  if (hpath) { q.A = nullptr; q.A_h = (const unsigned short*)w.pad; q.B_h = w.wcat_h; }
  q.B = w.wcat; q.ldb = kdim;
  q.C = c.dst;
  q.c_tab = w.t_ctab; q.sc_cout = c.cout; q.sc_wpitch = c.hb * c.cout;
  q.bias = c.bias; q.flags = c.flags; q.mulref = c.mulref; q.no_twin = c.no_twin;
  if (klist) {      // the lists written by convt_tables_launch
    q.k_list = klist; q.k_list_rows = CONVT_G; q.k_list_stride = dm_cdiv(kdim, 32) + 1;
    // the valid-tap share of the class grid: (ta hs)^2 of (ta Hc)^2
    q.k_list_mean = std::max(1.0, (double)dm_cdiv(kdim, 32) * c.hs * c.hs / ((double)Hc * Hc));
  }
  return dm_gemm_launch(q, splitk, DM_SPLITK_FLOATS * sizeof(float), st);
}

// ---------------------------------------------------------------- MSE (decoders.py:163-167) -----
// pred NHWC (n,hw,c), target NCHW (n,c,hw).  loss[n] = 0.5*sum (pred-target)^2 ; dpred = scale*(pred-target) (NHWC);
// rec = pred in NCHW.  One block per frame, fixed reduction order.
// U8: the target is the replay's uint8 HWC frame, converted on the fly (x/255 - 0.5); it shares the prediction's NHWC
// index, so both streams are coalesced.  tdiv: iwae_samples (decoders.py:163-167 expands the target over I: prediction
// frame i compares with target frame i / I);  row_scale (optional): per-frame factor on dpred (IWAE importance weights).
template <bool U8>
__global__ void __launch_bounds__(256) mse_image_kernel(int hw, int c, const float* __restrict__ pred,
                                                        const void* __restrict__ target_, int tdiv, float scale,
                                                        const float* __restrict__ row_scale,
                                                        float* __restrict__ loss, float* __restrict__ dpred, int dpad,
                                                        float* __restrict__ rec, unsigned short* __restrict__ dpred_h) {
  __shared__ float red[4];
  const int i = blockIdx.x;
  const int per = hw * c;
  const float* pr = pred + (size_t)i * per;
  const float* tg = (const float*)target_ + (size_t)(i / tdiv) * per;
  const uint8_t* tg8 = (const uint8_t*)target_ + (size_t)(i / tdiv) * per;
  if (row_scale) scale *= row_scale[i];
  float s = 0.f;
  for (int e = threadIdx.x; e < per; e += 256) {
    const int pix = e / c, cc = e % c;
    const float pv = pr[e];
    const float tv = U8 ? (float)tg8[e] / 255.0f - 0.5f : tg[(size_t)cc * hw + pix];
    const float d = pv - tv;
    s += d * d;
    if (dpred) {        // dpad >= c channels per pixel; the pad channels are written as zeros (see the 4-channel trick in backward)
      float* dp = dpred + ((size_t)i * hw + pix) * dpad;
      dp[cc] = scale * d;
      if (cc == c - 1)
        for (int q = c; q < dpad; ++q) dp[q] = 0.f;
      if (dpred_h) {      // bf16 twin of the gradient (common.h DmTwinScope)
        unsigned short* dh = dpred_h + ((size_t)i * hw + pix) * dpad;
        dh[cc] = (unsigned short)dm_f2bf(scale * d);
        if (cc == c - 1)
          for (int q = c; q < dpad; ++q) dh[q] = 0;
      }
    }
    if (rec) rec[(size_t)i * per + (size_t)cc * hw + pix] = pv;
  }
  s = dm_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0 && loss) loss[i] = 0.5f * (red[0] + red[1] + red[2] + red[3]);
}

// ---------------------------------------------------------------- uint8 ingest ---
// preprocessing.py:21-29 `to_image`: uint8 (n, h*w, c) HWC frames -> float32 (n, c, h*w) CHW in [-0.5, 0.5], x/255 - 0.5 in
// fp32 (correctly rounded division, same values as numpy's).  One pass: 1 byte read + 4 bytes written per element, so
// a replay batch crosses PCIe and HBM as 31 MB instead of 123 MB and the host-side astype/transposes disappear.
__global__ void __launch_bounds__(256) preprocess_u8_kernel(size_t n, int hw, int c, const uint8_t* __restrict__ src,
                                                            float* __restrict__ dst) {
  const size_t total = n * hw * c;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t i = e / ((size_t)hw * c);
    const int rem = (int)(e % ((size_t)hw * c));
    const int cc = rem / hw, pix = rem % hw;          // e indexes the CHW (output) side: coalesced writes
    dst[e] = (float)src[i * hw * c + (size_t)pix * c + cc] / 255.0f - 0.5f;
  }
}
extern "C" int dm_preprocess_image_u8(int64_t n, int hw, int c, const uint8_t* src, float* dst, void* stream) {
  DM_REQUIRE(src && dst, DM_E_NULL, "preprocess_image_u8: null pointer");
  DM_REQUIRE(n >= 0 && hw >= 1 && c >= 1, DM_E_SHAPE, "preprocess_image_u8: bad shape n=%lld hw=%d c=%d", (long long)n, hw, c);
  if (n == 0) return DM_OK;
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid_for((size_t)n * hw * c)), dim3(256), 0, (hipStream_t)stream, (size_t)n,
                     hw, c, src, dst);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

// dm_shape.flags bit 4: `image` / `target` pointers are uint8 (N, H, W, C) frames (the replay's native format)
static inline bool shape_u8(const dm_shape* s) { return (s->flags & DM_FLAG_IMAGE_U8) != 0; }
static int mse_launch(bool u8, int n, int hw, int c, const float* pred, const void* target, int tdiv, float scale,
                      const float* row_scale, float* loss, float* dpred, int dpad, float* rec, hipStream_t st) {
  unsigned short* dh = dpred ? dm_twin_of(dpred, false) : nullptr;      // bf16 mode: the gradient's twin, written here
  if (dh) dm_twin_mark(dpred);
  if (u8) hipLaunchKernelGGL((mse_image_kernel<true>), dim3(n), dim3(256), 0, st, hw, c, pred, target, tdiv, scale, row_scale, loss, dpred, dpad, rec, dh);
  else hipLaunchKernelGGL((mse_image_kernel<false>), dim3(n), dim3(256), 0, st, hw, c, pred, target, tdiv, scale, row_scale, loss, dpred, dpad, rec, dh);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

// ---------------------------------------------------------------- geometry ----------------------
struct EncGeom {
  int N, ch, d;
  int hb[4], hs[4], cin[4], cout[4];
  size_t rows[4], kdim[4];
  bool direct0;      // layer 1 runs as a direct convolution (conv_direct.hip): no explicit patch matrix
  bool twins;        // bf16 mode: the arena also holds bf16 twins of y[0..2] and of the repacked weights (common.h DmTwinScope)
  explicit EncGeom(const dm_shape* s) {
    twins = (s->flags & DM_FLAG_BF16) != 0;
    N = s->T * s->B * (s->I > 0 ? s->I : 1);
    ch = s->img_ch; d = s->cnn_depth;
    direct0 = dm_enc_l1_direct_ok(ch, d, s->img);
    int h = s->img;
    const int ci[4] = {ch, d, 2 * d, 4 * d};
    const int co[4] = {d, 2 * d, 4 * d, 8 * d};
    for (int l = 0; l < 4; ++l) {
      hb[l] = h;
      hs[l] = (h - 4) / 2 + 1;
      cin[l] = ci[l]; cout[l] = co[l];
      rows[l] = (size_t)N * hs[l] * hs[l];
      kdim[l] = (size_t)16 * ci[l];
      h = hs[l];
    }
  }
  bool valid(const dm_shape* s) const {
    return s->img == 64 && hs[3] == 2 && s->E == 8 * d * 4 && ch >= 1 && d >= 1;
  }
  bool valid_planes(const dm_shape* s) const { return s->img == 64 && hs[3] == 2 && direct0; }      // reward_input: E is the caller's
};

struct DecGeom {
  int N, ch, d, F;
  int k[5], hsm[5], hbg[5], cin[5], cout[5];   // index 1..4
  size_t rows_s[5], rows_b[5];
  bool twins;       // bf16 mode: the arena also holds bf16 twins of x[0..2] and wr[1..4] (common.h DmTwinScope)
  explicit DecGeom(const dm_shape* s) {
    twins = (s->flags & DM_FLAG_BF16) != 0;
    N = s->T * s->B * (s->I > 0 ? s->I : 1);
    ch = s->img_ch; d = s->cnn_depth;
    F = s->D + s->S * (s->C ? s->C : 1);      // Gaussian latents (C = 0) are S wide
    const int kk[5] = {0, 5, 5, 6, 6};
    const int ci[5] = {0, 32 * d, 4 * d, 2 * d, d};
    const int co[5] = {0, 4 * d, 2 * d, d, ch};
    int h = 1;
    for (int l = 1; l <= 4; ++l) {
      k[l] = kk[l]; cin[l] = ci[l]; cout[l] = co[l];
      hsm[l] = h;
      hbg[l] = 2 * (h - 1) + kk[l];
      rows_s[l] = (size_t)N * h * h;
      rows_b[l] = (size_t)N * hbg[l] * hbg[l];
      h = hbg[l];
    }
  }
  bool valid(const dm_shape* s) const { return hbg[4] == s->img && s->img == 64; }
};
static bool dec_direct4(const DecGeom& g) { return dm_dec_l4_direct_ok(g.ch, g.d, g.hsm[4], g.k[4]); }      // the shape admits the image layer's direct kernels

// ---------------------------------------------------------------- plans -------------------------
// What an entry point does at a shape.  enc_fwd_plan / enc_bwd_plan / dec_fwd_plan / dec_bwd_plan compute it from the geometry,
// `planes`, whether bf16 twins are in use (tw_on) and the process switches - no HIP call, no pointer read; the launch loops only
// carry out form[l], and the layouts size from the same plan (include/dreamer_hip.h dm_conv_plan_query lists the codes).
enum { CONV_DIRECT = 0, CONV_DIRECT_PLANES = 1, CONV_PATCH = 2, CONV_IMPLICIT = 3, CONV_GATHER = 4, CONV_COLUMN = 5, CONV_ONE_PIXEL = 6 };
enum { CONV_HPATH = 1, CONV_PADDED = 2, CONV_REPITCH = 4 };
struct ConvPlan {
  int form[5] = {-1, -1, -1, -1, -1}, bits[5] = {0, 0, 0, 0, 0};      // by layer: encoder 0..3, decoder 1..4
  bool kskip = false;          // gather layers: chunk-major rows and k-tile lists (dm_convt_kskip_enable, fp32 only)
  ConvtScratch gather;         // scratch of the gather layers, folded
  size_t need = 0;             // workspace, floats
  // layer l as a gather-form layer, if admitted; CONV_HPATH: its padded operand and weights are stored as bf16
  bool take_gather(int l, bool tw_on, int k, int cin, int cout, int hs, size_t n) {
    const ConvtScratch s = convt_gather_scratch(k, cin, cout, hs, n);
    if (!s.ok) return false;
    form[l] = CONV_GATHER;
    bits[l] = tw_on && (cin & 7) == 0 && (k / 2) * (k / 2) * cin >= DM_HSTORE_MIN_K ? CONV_HPATH : 0;
    gather.fold(s);
    return true;
  }
};

// ---------------------------------------------------------------- encoder -----------------------
struct EncActs {
  float* wr[4];    // repacked weights (l>=1)
  float* xcol[4];  // explicit patch matrix: layer 0 only (reads the NCHW batch, 3 channels)
  int* rowoff[4];  // implicit-im2col tables (l>=1), see conv_tables_kernel
  int* koff[4];
  float* y[4];     // post-ELU NHWC outputs
  unsigned short* yh[4];    // bf16 mode: twins of y[0..2] and wr[1..3], behind everything else (fp32 offsets do not move)
  unsigned short* wrh[4];
};
static size_t enc_carve(const EncGeom& g, float* base, size_t cap_floats, EncActs* a) {
  DmArena ar(base, cap_floats * sizeof(float));
  for (int l = 0; l < 4; ++l) {
    float* w = ar.take(l == 0 ? 0 : (size_t)g.cout[l] * g.kdim[l]);
    float* xc = ar.take(l == 0 && !g.direct0 ? g.rows[l] * g.kdim[l] : 0);
    float* ro = ar.take(l == 0 ? 0 : g.rows[l]);
    float* ko = ar.take(l == 0 ? 0 : g.kdim[l]);
    float* yy = ar.take(g.rows[l] * g.cout[l]);
    if (a) { a->wr[l] = w; a->xcol[l] = xc; a->rowoff[l] = (int*)ro; a->koff[l] = (int*)ko; a->y[l] = yy; }
  }
  for (int l = 0; l < 4; ++l) {
    float* yh = ar.take(g.twins && l < 3 ? dm_half_floats(g.rows[l] * g.cout[l]) : 0);
    float* wh = ar.take(g.twins && l > 0 ? dm_half_floats((size_t)g.cout[l] * g.kdim[l]) : 0);
    if (a) { a->yh[l] = (unsigned short*)yh; a->wrh[l] = (unsigned short*)wh; }
  }
  return ar.off;
}
static void enc_register_twins(const EncGeom& g, const EncActs& a, bool acts_valid, bool weights_valid) {
  if (!dm_twins_on()) return;
  for (int l = 0; l < 3; ++l) dm_twin_add(a.y[l], g.rows[l] * g.cout[l], a.yh[l], acts_valid);
  for (int l = 1; l < 4; ++l) dm_twin_add(a.wr[l], (size_t)g.cout[l] * g.kdim[l], a.wrh[l], weights_valid);
}
extern "C" size_t dm_conv_encoder_acts_floats(const dm_shape* shp) {
  if (!shp) return 0;
  EncGeom g(shp);
  return enc_carve(g, nullptr, 0, nullptr);
}

// NHWC (n, hw, c) <-> torch flatten order (n, c*hw + pix)
__global__ void __launch_bounds__(256) nhwc_to_chw_flat_kernel(size_t n, int hw, int c, const float* __restrict__ src,
                                                               float* __restrict__ dst, int to_chw) {
  const size_t total = n * hw * c;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t i = e / ((size_t)hw * c);
    const int rem = (int)(e % ((size_t)hw * c));
    const int pix = rem / c, cc = rem % c;        // e indexes the NHWC side
    const size_t o = i * hw * c + (size_t)cc * hw + pix;
    if (to_chw) dst[o] = src[e];
    else dst[e] = src[o];
  }
}

// the same with a leading dimension on the torch side: row i of it starts at i * ld (ld >= hw * c)
__global__ void __launch_bounds__(256) nhwc_to_chw_flat_ld_kernel(size_t n, int hw, int c, const float* __restrict__ src,
                                                                  float* __restrict__ dst, int ld, int to_chw) {
  const size_t total = n * hw * c;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t i = e / ((size_t)hw * c);
    const int rem = (int)(e % ((size_t)hw * c));
    const int pix = rem / c, cc = rem % c;        // e indexes the NHWC side
    if (to_chw) dst[i * ld + (size_t)cc * hw + pix] = src[e];
    else dst[e] = src[i * ld + (size_t)cc * hw + pix];
  }
}

// the embedding (n, 4 c) in torch's flatten order, leading dimension ld, to (to_chw = 0: from) the NHWC layer-4 tensor
static int chw_flat_launch(size_t n, int c, const float* src, float* dst, int ld, int to_chw, hipStream_t st) {
  if (ld == 4 * c)
    hipLaunchKernelGGL(nhwc_to_chw_flat_kernel, dim3(grid_for(n * 4 * c)), dim3(256), 0, st, n, 4, c, src, dst, to_chw);
  else
    hipLaunchKernelGGL(nhwc_to_chw_flat_ld_kernel, dim3(grid_for(n * 4 * c)), dim3(256), 0, st, n, 4, c, src, dst, ld, to_chw);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
// The geometry both directions accept.  planes (reward_input): E is the caller's, ld the leading dimension of the embedding.
static int enc_validate(const dm_shape* shp, const EncGeom& g, bool planes, int ld, const char* what) {
  DM_REQUIRE((planes ? g.valid_planes(shp) : g.valid(shp)) && ld >= 32 * g.d, DM_E_SHAPE,
             "%s: unsupported geometry (img=%d, ch=%d, E=%d, depth=%d, ld=%d, planes=%d: built for 3 x 64 x 64 frames and cnn_depth in "
             "{8,16,32,48,64})", what, shp->img, shp->img_ch, shp->E, shp->cnn_depth, ld, (int)planes);
  return DM_OK;
}

// The forward's workspace: [split-K | the direct layer-1 kernel's transposed weights | reward_input: its per-frame bias].  On an
// arena without a base it sizes.
struct EncFwdWs { float *splitk, *wt, *fb; };
static size_t enc_fwd_layout(DmArena ar, const EncGeom& g, const ConvPlan& pl, bool planes, EncFwdWs* w) {
  w->splitk = ar.take(DM_SPLITK_FLOATS);
  w->wt = ar.take(pl.form[0] == CONV_DIRECT ? (size_t)48 * g.d : 0);
  w->fb = ar.take(planes ? (size_t)g.N * g.d : 0);
  return ar.off;
}
static ConvPlan enc_fwd_plan(const EncGeom& g, bool planes) {
  ConvPlan pl;
  pl.form[0] = g.direct0 ? CONV_DIRECT : CONV_PATCH;      // 3 -> d channels: one direct kernel on the frame / an explicit patch matrix
  for (int l = 1; l < 4; ++l) pl.form[l] = CONV_IMPLICIT;
  EncFwdWs w;
  pl.need = enc_fwd_layout(DmArena(nullptr, 0), g, pl, planes, &w);
  return pl;
}

// reward / terminal (N,): non-null = reward_input, p->w[0] is (d, 5, 4, 4) and the two planes are folded into layer 1
// (conv_direct.hip); ld: leading dimension of `embed` (the caller may keep other encoders' outputs behind the image embedding)
static int conv_encoder_fwd_impl(const dm_shape* shp, const float* image, const dm_conv_params* p, float* acts, float* embed,
                                 int ld, const float* reward, const float* terminal, void* ws, size_t ws_bytes, void* stream) {
  DmPrecisionScope prec(shp->flags & DM_FLAG_BF16);
  EncGeom g(shp);
  const bool planes = reward != nullptr;
  DM_TRY(enc_validate(shp, g, planes, ld, "conv_encoder_fwd"));
  hipStream_t st = (hipStream_t)stream;
  EncActs a;
  enc_carve(g, acts, (size_t)1 << 60, &a);
  const ConvPlan pl = enc_fwd_plan(g, planes);
  EncFwdWs w;
  enc_fwd_layout(DmArena(ws, ws_bytes), g, pl, planes, &w);
  DM_REQUIRE(pl.need <= ws_bytes / sizeof(float), DM_E_WORKSPACE, "conv_encoder_fwd: workspace too small (need %zu floats)", pl.need);
  DmTwinScope tw((shp->flags & DM_FLAG_BF16) != 0);
  enc_register_twins(g, a, false, false);
  dm_twin_arena_note(acts, dm_twins_on());
  for (int l = 1; l < 4; ++l) {
    DM_TRY(conv_tables_launch(g.N, g.hb[l], g.hb[l], g.cin[l], 4, a.rowoff[l], a.koff[l], st));
    DM_TRY(dm_permute4_launch(p->w[l], a.wr[l], g.cout[l], g.cin[l], 4, 4, 0, 2, 3, 1, st));
  }
  if (dm_twins_on()) {
    DmCvtSeg sg[3];
    for (int l = 1; l < 4; ++l) { sg[l - 1] = DmCvtSeg{a.wr[l], a.wrh[l], (size_t)g.cout[l] * g.kdim[l]}; dm_twin_mark(a.wr[l]); }
    DM_TRY(dm_to_bf16_multi_launch(sg, 3, st));
  }
  if (g.N == 0) return DM_OK;
  for (int l = 0; l < 4; ++l) switch (pl.form[l]) {
    case CONV_DIRECT: {      // no patch matrix (conv_direct.hip)
      unsigned short* y0h = dm_twin_of(a.y[0], false);
      if (planes)
        DM_TRY(dm_enc_l1_fwd_planes_launch(g.N, g.d, shape_u8(shp) ? 1 : 0, image, p->w[0], p->b[0], reward, terminal, w.wt, w.fb,
                                           a.y[0], y0h, st));
      else
        DM_TRY(dm_enc_l1_fwd_launch(g.N, g.d, shape_u8(shp) ? 1 : 0, image, p->w[0], p->b[0], w.wt, a.y[0], y0h, st));
      if (y0h) dm_twin_mark(a.y[0]);
      break;
    }
    case CONV_PATCH:
      if (shape_u8(shp)) {
        const size_t total = (size_t)g.N * g.hs[0] * g.hs[0] * g.kdim[0];
        hipLaunchKernelGGL(im2col_s2_u8hwc_kernel, dim3(grid_for(total)), dim3(256), 0, st, g.N, g.hb[0], g.hb[0], g.cin[0], 4,
                           g.hs[0], g.hs[0], (const uint8_t*)image, a.xcol[0]);
        DM_LAUNCH_CHECK();
      } else {
        DM_TRY(dm_im2col_s2_launch(g.N, g.hb[0], g.hb[0], g.cin[0], 4, image, 1, a.xcol[0], st));
      }
      [[fallthrough]];      // the product over the patch matrix: explicit here, gathered from the layer below otherwise
    default: {
      DmGemm q;
      q.a_layout = 0; q.b_layout = 0;
      q.M = g.N * g.hs[l] * g.hs[l]; q.N = g.cout[l]; q.K = (int)g.kdim[l];
      if (l == 0) { q.A = a.xcol[0]; q.lda = q.K; }
      else {
        q.A = a.y[l - 1]; q.a_maj = a.rowoff[l]; q.a_min = a.koff[l];
        q.a_tab_vec = (g.cin[l] & 3) == 0; q.a_tab_vec8 = (g.cin[l] & 7) == 0;
      }
      q.B = l == 0 ? p->w[0] : a.wr[l]; q.ldb = q.K;
      q.C = a.y[l]; q.ldc = q.N;
      q.bias = p->b[l];
      q.flags = DM_GEMM_ELU;
      DM_TRY(dm_gemm_launch(q, w.splitk, DM_SPLITK_FLOATS * sizeof(float), st));
    }
  }
  return chw_flat_launch((size_t)g.N, g.cout[3], a.y[3], embed, ld, 1, st);
}
extern "C" int dm_conv_encoder_fwd(const dm_shape* shp, const float* image, const dm_conv_params* p, float* acts,
                                   float* embed, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(shp && image && p && acts && embed && ws, DM_E_NULL, "conv_encoder_fwd: null pointer");
  return conv_encoder_fwd_impl(shp, image, p, acts, embed, 32 * shp->cnn_depth, nullptr, nullptr, ws, ws_bytes, stream);
}
extern "C" int dm_conv_encoder_fwd_planes(const dm_shape* shp, const float* image, const dm_conv_params* p,
                                          const float* reward, const float* terminal, float* acts, float* embed, int ld_embed,
                                          void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(shp && image && p && acts && embed && ws && !reward == !terminal, DM_E_NULL, "conv_encoder_fwd_planes: null pointer");
  return conv_encoder_fwd_impl(shp, image, p, acts, embed, ld_embed, reward, terminal, ws, ws_bytes, stream);
}

// The backward's workspace.  ga / gb: the gradient ping-pong (ga holds the largest, layer 1's output gradient); dwr: a weight
// gradient in the repacked layout; dxcol: the explicit patch-matrix gradient of the layers that do not take the gather form,
// and the direct layer-1 kernels' partials.  On an arena without a base it sizes.
struct EncBwdWs {
  float *splitk, *ga, *gb, *dwr, *dxcol;
  ConvtWs gather;      // the gather-form data gradients (the data gradient of a stride-2 convolution IS a transposed convolution)
  unsigned short *ga_h, *gb_h; size_t gmax, xcmax;      // floats of ga and of dxcol
};
static size_t enc_bwd_layout(DmArena ar, const EncGeom& g, const ConvPlan& pl, bool tw_on, EncBwdWs* w) {
  w->splitk = ar.take(DM_SPLITK_FLOATS);
  const size_t gmax = w->gmax = g.rows[0] * g.cout[0];
  w->ga = ar.take(gmax);
  w->gb = ar.take(g.rows[1] * g.cout[1]);
  w->dwr = ar.take((size_t)g.cout[3] * g.kdim[3]);
  size_t xcmax = 0;
  for (int l = 1; l < 4; ++l) if (g.rows[l] * g.kdim[l] > xcmax) xcmax = g.rows[l] * g.kdim[l];
  w->dxcol = ar.take(w->xcmax = xcmax);
  convt_gather_carve(ar, pl.gather, 4 * 1024, tw_on, &w->gather);      // k = 4: K = 4 cout, up to 1024 output channels
  // bf16 mode: twins of the two gradient ping-pong buffers (the padded gradient copy is written as bf16 only, in the fp32 copy's storage)
  w->ga_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(gmax) : 0);
  w->gb_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(g.rows[1] * g.cout[1]) : 0);
  return ar.off;
}
static ConvPlan enc_bwd_plan(const EncGeom& g, bool planes, bool tw_on) {
  ConvPlan pl;
  pl.kskip = g_convt_kskip && !g.twins;
  pl.form[0] = !g.direct0 ? CONV_PATCH : planes ? CONV_DIRECT_PLANES : CONV_DIRECT;      // layer 0 has a weight gradient only
  for (int l = 1; l < 4; ++l)      // the data gradient out of layer l: a (cout -> cin) transposed convolution from hs to hb
    if (!pl.take_gather(l, tw_on, 4, g.cout[l], g.cin[l], g.hs[l], (size_t)g.N)) pl.form[l] = CONV_COLUMN;
  EncBwdWs w;
  pl.need = enc_bwd_layout(DmArena(nullptr, 0), g, pl, tw_on, &w);
  return pl;
}

static int conv_encoder_bwd_impl(const dm_shape* shp, const float* image, const dm_conv_params* p, const float* acts,
                                 const float* dembed, int ld, const float* reward, const float* terminal, const dm_conv_grads* gr,
                                 void* ws, size_t ws_bytes, void* stream) {
  DmPrecisionScope prec(shp->flags & DM_FLAG_BF16);
  EncGeom g(shp);
  const bool planes = reward != nullptr;
  DM_TRY(enc_validate(shp, g, planes, ld, "conv_encoder_bwd"));
  hipStream_t st = (hipStream_t)stream;
  EncActs a;
  enc_carve(g, const_cast<float*>(acts), (size_t)1 << 60, &a);
  DmTwinScope tw((shp->flags & DM_FLAG_BF16) != 0);
  const bool tw_on = dm_twins_on();
  const ConvPlan pl = enc_bwd_plan(g, planes, tw_on);
  EncBwdWs w;
  enc_bwd_layout(DmArena(ws, ws_bytes), g, pl, tw_on, &w);
  DM_REQUIRE(pl.need <= ws_bytes / sizeof(float), DM_E_WORKSPACE, "conv_encoder_bwd: workspace too small (need %zu floats)", pl.need);
  const auto& [splitk, ga, gb, dwr, dxcol, gather, ga_h, gb_h, gmax, xcmax] = w;
  const size_t skb = DM_SPLITK_FLOATS * sizeof(float);
  const bool arena_tw = dm_twin_arena_valid(acts);      // the forward that filled `acts` wrote its twins
  enc_register_twins(g, a, arena_tw, arena_tw);
  dm_twin_add(ga, gmax, ga_h, false);
  dm_twin_add(gb, g.rows[1] * g.cout[1], gb_h, false);

  // dY3 (NHWC) = permute(dembed) ; G = dY3 * ELU'(Y3)
  float* G = gb;      // layer-3 grads are small; ping-pong between ga / gb going down
  const size_t tot3 = (size_t)g.N * 4 * g.cout[3];
  DM_TRY(chw_flat_launch((size_t)g.N, g.cout[3], dembed, G, ld, 0, st));
  DM_TRY(dm_mul_elu_grad_launch(tot3, G, a.y[3], G, st));
  if (tw_on) {
    const DmCvtSeg sg = {G, dm_twin_of(G, false), tot3};
    DM_TRY(dm_to_bf16_multi_launch(&sg, 1, st));
    dm_twin_mark(G);
  }
  for (int l = 3; l >= 0; --l) {
    const int rows = (int)g.rows[l], co = g.cout[l], kd = (int)g.kdim[l];
    const bool with_planes = pl.form[l] == CONV_DIRECT_PLANES;
    if (!with_planes) DM_TRY(dm_colsum_launch(rows, co, G, co, gr->b[l], splitk, skb, st));
    if (with_planes || pl.form[l] == CONV_DIRECT) {      // patches re-gathered from the frame inside the weight-gradient kernel (conv_direct.hip)
      // reward_input: the image channels' weight gradient as ever (into `dwr`, free by now), then ONE frame-weighted column sum
      // over G gives the bias gradient and the two plane gradients, and the (d, 5, 4, 4) gradient is assembled
      DM_REQUIRE(image, DM_E_NULL, "conv_encoder_bwd: the direct layer-1 weight gradient reads the image");
      DM_REQUIRE(dm_enc_l1_wgrad_part_floats(g.N, g.d) <= xcmax && (!with_planes || dm_enc_l1_planes_part_floats(g.N, g.d) <= xcmax),
                 DM_E_WORKSPACE, "conv_encoder_bwd: partial buffer too small");
      DM_TRY(dm_enc_l1_wgrad_launch(g.N, g.d, shape_u8(shp) ? 1 : 0, image, G, dxcol, with_planes ? dwr : gr->w[0], splitk, skb, st));
      if (with_planes) DM_TRY(dm_enc_l1_planes_bwd_launch(g.N, g.d, G, reward, terminal, dwr, dxcol, gr->b[0], gr->w[0], st));
      break;
    }
    DmGemm q;   // dWr[o][kidx] = sum_rows G[row][o] * Xcol[row][kidx]
    q.a_layout = 1; q.b_layout = 1;
    q.M = co; q.N = kd; q.K = rows;
    q.A = G; q.lda = co;
    if (l == 0) { q.B = a.xcol[0]; q.ldb = kd; }
    else {
      q.B = a.y[l - 1]; q.b_maj = a.rowoff[l]; q.b_min = a.koff[l];
      q.b_tab_vec = (g.cin[l] & 3) == 0; q.b_tab_vec8 = (g.cin[l] & 7) == 0;
    }
    q.C = (l == 0) ? gr->w[0] : dwr; q.ldc = kd;
    DM_TRY(dm_gemm_launch(q, splitk, skb, st));
    if (l == 0) break;
    DM_TRY(dm_permute4_launch(dwr, gr->w[l], co, 4, 4, g.cin[l], 0, 3, 1, 2, st));
    float* Gn = (l == 1 || G != ga) ? ga : gb;      // ping-pong; layer 0's output gradient, the largest, goes to ga
    if (pl.form[l] == CONV_GATHER) {
      // dX[n, 2yy+py, 2xx+px, i] = ELU'(Y_{l-1}) * sum_{a,b,o} G[n, yy-a, xx-b, o] W[o][i][py+2a][px+2b]: one implicit GEMM
      // over a zero-padded copy of G, scattered straight into the NHWC gradient of layer l-1 (no dXcol, no col2im)
      ConvtGather c = {"conv_encoder_bwd", g.N, g.hs[l], g.hb[l], 4, co, g.cin[l], G, p->w[l], Gn};
      c.mulref = a.y[l - 1];
      c.no_twin = l == 1;      // the layer-0 gradient is read by the direct weight-gradient kernel and the bias sum only (fp32)
      DM_TRY(convt_gather_launch(c, gather, pl.bits[l] & CONV_HPATH, pl.kskip, splitk, st));
    } else {
      DmGemm d;   // dXcol[row][kidx] = sum_o G[row][o] * Wr[o][kidx]
      d.a_layout = 0; d.b_layout = 1;
      d.M = rows; d.N = kd; d.K = co;
      d.A = G; d.lda = co;
      d.B = a.wr[l]; d.ldb = kd;
      d.C = dxcol; d.ldc = kd;
      DM_TRY(dm_gemm_launch(d, splitk, skb, st));
      DM_TRY(dm_col2im_s2_launch(g.N, g.hb[l], g.hb[l], g.cin[l], 4, dxcol, nullptr, 0, a.y[l - 1], Gn, st));
    }
    G = Gn;
  }
  return DM_OK;
}
extern "C" int dm_conv_encoder_bwd(const dm_shape* shp, const float* image, const dm_conv_params* p, const float* acts,
                                   const float* dembed, const dm_conv_grads* gr, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(shp && p && acts && dembed && gr && ws, DM_E_NULL, "conv_encoder_bwd: null pointer");
  return conv_encoder_bwd_impl(shp, image, p, acts, dembed, 32 * shp->cnn_depth, nullptr, nullptr, gr, ws, ws_bytes, stream);
}
extern "C" int dm_conv_encoder_bwd_planes(const dm_shape* shp, const float* image, const dm_conv_params* p,
                                          const float* reward, const float* terminal, const float* acts, const float* dembed,
                                          int ld_dembed, const dm_conv_grads* gr, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(shp && p && acts && dembed && gr && ws && !reward == !terminal && (image || !reward), DM_E_NULL,
             "conv_encoder_bwd_planes: null pointer");
  return conv_encoder_bwd_impl(shp, image, p, acts, dembed, ld_dembed, reward, terminal, gr, ws, ws_bytes, stream);
}

// 4-channel trick for the image layer's backward (cout = 3): the output gradient is written with 4 channels per pixel (the
// 4th = 0) and the weights are padded to match, so its patches are 16-byte gathers like every other layer's and the
// explicit patch matrix of the 3-channel gradient (972 MB written + read at Atari-literal) is never built.
// dst (I, k, k, O4) <- src (I, O, k, k)  (torch ConvTranspose2d layout), zero for o >= O
__global__ void __launch_bounds__(256) convt_pad_cout_kernel(int I, int O, int O4, int k, const float* __restrict__ src,
                                                             float* __restrict__ dst) {
  const int total = I * k * k * O4;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int o = e % O4, kx = (e / O4) % k, ky = (e / (O4 * k)) % k, i = e / (O4 * k * k);
    dst[e] = o < O ? src[(((size_t)i * O + o) * k + ky) * k + kx] : 0.f;
  }
}
// dst (I, O, k, k) <- src (I, k, k, O4), dropping the pad channels
__global__ void __launch_bounds__(256) convt_unpad_cout_kernel(int I, int O, int O4, int k, const float* __restrict__ src,
                                                               float* __restrict__ dst) {
  const int total = I * O * k * k;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int kx = e % k, ky = (e / k) % k, o = (e / (k * k)) % O, i = e / (k * k * O);
    dst[e] = src[(((size_t)i * k + ky) * k + kx) * O4 + o];
  }
}

// ---------------------------------------------------------------- decoder -----------------------
struct DecActs {
  float* wr[5];
  float* x[5];     // x[0] = fc output (N,32d); x[l] = NHWC activations after layer l (x[4] = prediction)
  unsigned short* xh[5];     // bf16 mode: twins of x[0..2] and wr[1..4], behind everything else (dm_conv_decoder_pred_offset holds)
  unsigned short* wrh[5];
  size_t pred_off;           // float offset of x[4] in the arena
};
static inline size_t dec_x_elems(const DecGeom& g, int l) { return l == 0 ? (size_t)g.N * g.cin[1] : g.rows_b[l] * g.cout[l]; }
static inline size_t dec_w_elems(const DecGeom& g, int l) { return (size_t)g.cin[l] * g.k[l] * g.k[l] * g.cout[l]; }
static size_t dec_carve(const DecGeom& g, float* base, size_t cap_floats, DecActs* a) {
  DmArena ar(base, cap_floats * sizeof(float));
  float* x0 = ar.take((size_t)g.N * g.cin[1]);
  if (a) a->x[0] = x0;
  for (int l = 1; l <= 4; ++l) {
    float* w = ar.take((size_t)g.cin[l] * g.k[l] * g.k[l] * g.cout[l]);
    if (a && l == 4) a->pred_off = ar.off;
    float* xx = ar.take(g.rows_b[l] * g.cout[l]);
    if (a) { a->wr[l] = w; a->x[l] = xx; }
  }
  for (int l = 0; l <= 4; ++l) {
    float* xh = ar.take(g.twins && l < 3 ? dm_half_floats(dec_x_elems(g, l)) : 0);
    float* wh = ar.take(g.twins && l > 0 ? dm_half_floats(dec_w_elems(g, l)) : 0);
    if (a) { a->xh[l] = (unsigned short*)xh; a->wrh[l] = (unsigned short*)wh; }
  }
  return ar.off;
}
static void dec_register_twins(const DecGeom& g, const DecActs& a, bool acts_valid, bool weights_valid) {
  if (!dm_twins_on()) return;
  // (x[3], the 30x30xd input of the image layer, gets none: writing it costs more than its one reader, that layer's weight gradient, gains)
  for (int l = 0; l < 3; ++l) dm_twin_add(a.x[l], dec_x_elems(g, l), a.xh[l], acts_valid);
  for (int l = 1; l <= 4; ++l) dm_twin_add(a.wr[l], dec_w_elems(g, l), a.wrh[l], weights_valid);
}
extern "C" size_t dm_conv_decoder_acts_floats(const dm_shape* shp) {
  if (!shp) return 0;
  DecGeom g(shp);
  return dec_carve(g, nullptr, 0, nullptr);
}

// Float offset, inside the `acts` buffer of dm_conv_decoder_mse_fwd, of the decoder's prediction (N, img, img, ch) NHWC:
// lets the caller materialise `image_rec` (decoders.py:177) only when somebody reads it.
extern "C" size_t dm_conv_decoder_pred_offset(const dm_shape* shp) {
  if (!shp) return 0;
  DecGeom g(shp);
  DecActs a;
  dec_carve(g, nullptr, 0, &a);
  return a.pred_off;
}

// The forward's workspace.  ycol: the column matrix of the layers that take neither the gather form nor (image layer) the
// direct kernel; w4: that kernel's class-ordered weights; then the gather form's block.  On an arena without a base it sizes.
struct DecFwdWs { float *splitk, *ycol, *w4; ConvtWs gather; };
static size_t dec_fwd_layout(DmArena ar, const DecGeom& g, const ConvPlan& pl, bool tw_on, DecFwdWs* w) {
  w->splitk = ar.take(DM_SPLITK_FLOATS);
  size_t colmax = 0;      // (sized over every layer that is not direct, whatever form it takes)
  for (int l = 1; l <= 4; ++l)
    if (pl.form[l] != CONV_DIRECT) colmax = std::max(colmax, g.rows_s[l] * g.k[l] * g.k[l] * g.cout[l]);
  w->ycol = ar.take(colmax);
  w->w4 = ar.take(pl.form[4] == CONV_DIRECT ? dm_dec_l4_w4_floats(g.d) : 0);
  convt_gather_carve(ar, pl.gather, 9 * 1024, tw_on, &w->gather);      // k <= 6: K = 9 cin, up to 1024 input channels
  return ar.off;
}
static ConvPlan dec_fwd_plan(const DecGeom& g, bool tw_on) {
  ConvPlan pl;
  pl.kskip = g_convt_kskip && !g.twins;
  for (int l = 1; l <= 4; ++l)
    if (l == 4 && dec_direct4(g)) pl.form[l] = CONV_DIRECT;      // d -> 3 channels: conv_direct.hip, no column matrix
    else if (!pl.take_gather(l, tw_on, g.k[l], g.cin[l], g.cout[l], g.hsm[l], (size_t)g.N))
      pl.form[l] = g.hsm[l] == 1 ? CONV_ONE_PIXEL : CONV_COLUMN;      // a 1x1 input: no windows overlap, the column matrix IS the NHWC output
  DecFwdWs w;
  pl.need = dec_fwd_layout(DmArena(nullptr, 0), g, pl, tw_on, &w);
  return pl;
}

extern "C" int dm_conv_decoder_mse_fwd(const dm_shape* shp, const float* feat, int ldf, const float* target,
                                       const dm_conv_params* p, float* acts, float* loss_image, float* image_rec,
                                       void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(shp && feat && target && p && acts && ws, DM_E_NULL, "conv_decoder_fwd: null pointer");
  DmPrecisionScope prec(shp->flags & DM_FLAG_BF16);
  DecGeom g(shp);
  DM_REQUIRE(g.valid(shp), DM_E_SHAPE, "conv_decoder: unsupported geometry (img=%d)", shp->img);
  const int n = g.N;
  hipStream_t st = (hipStream_t)stream;
  DecActs a;
  dec_carve(g, acts, (size_t)1 << 60, &a);
  DmTwinScope tw((shp->flags & DM_FLAG_BF16) != 0);
  const bool tw_on = dm_twins_on();
  dec_register_twins(g, a, false, false);
  const ConvPlan pl = dec_fwd_plan(g, tw_on);
  DecFwdWs w;
  dec_fwd_layout(DmArena(ws, ws_bytes), g, pl, tw_on, &w);
  DM_REQUIRE(pl.need <= ws_bytes / sizeof(float), DM_E_WORKSPACE, "conv_decoder_fwd: workspace too small (need %zu floats)", pl.need);
  dm_twin_arena_note(acts, tw_on);
  for (int l = 1; l <= 4; ++l)
    DM_TRY(dm_permute4_launch(p->w[l], a.wr[l], g.cin[l], g.cout[l], g.k[l], g.k[l], 0, 2, 3, 1, st));
  if (tw_on) {
    DmCvtSeg sg[4];
    for (int l = 1; l <= 4; ++l) { sg[l - 1] = DmCvtSeg{a.wr[l], a.wrh[l], dec_w_elems(g, l)}; dm_twin_mark(a.wr[l]); }
    DM_TRY(dm_to_bf16_multi_launch(sg, 4, st));
  }
  if (n == 0) return DM_OK;
  const auto& [splitk, ycol, w4, gather] = w;
  const size_t skb = DM_SPLITK_FLOATS * sizeof(float);
  {
    DmGemm q;   // x0 = feat W^T + b
    q.M = n; q.N = g.cin[1]; q.K = g.F;
    q.A = feat; q.lda = ldf;
    q.B = p->w[0]; q.ldb = g.F;
    q.C = a.x[0]; q.ldc = q.N;
    q.bias = p->b[0];
    DM_TRY(dm_gemm_launch(q, splitk, skb, st));
  }
  for (int l = 1; l <= 4; ++l) {
    const float* xin = a.x[l - 1];
    if (pl.form[l] == CONV_DIRECT) {
      DM_TRY(dm_dec_l4_fwd_launch(n, g.d, xin, p->w[4], p->b[4], w4, a.x[4], st));
    } else if (pl.form[l] == CONV_GATHER) {
      ConvtGather c = {"conv_decoder_fwd", n, g.hsm[l], g.hbg[l], g.k[l], g.cin[l], g.cout[l], xin, p->w[l], a.x[l]};
      c.bias = p->b[l];
      c.flags = l < 4 ? DM_GEMM_ELU : 0;
      DM_TRY(convt_gather_launch(c, gather, pl.bits[l] & CONV_HPATH, pl.kskip, splitk, st));
    } else {
      const bool one = pl.form[l] == CONV_ONE_PIXEL;      // bias + ELU in the epilogue, straight into x[l]
      DmGemm q;   // Ycol[(n,ys,xs)][(ky,kx,o)] = X[(n,ys,xs)][i] * Wr[i][(ky,kx,o)]
      q.a_layout = 0; q.b_layout = 1;
      q.M = n * g.hsm[l] * g.hsm[l]; q.N = g.k[l] * g.k[l] * g.cout[l]; q.K = g.cin[l];
      q.A = xin; q.lda = q.K;
      q.B = a.wr[l]; q.ldb = q.N;
      q.C = one ? a.x[l] : ycol; q.ldc = q.N;
      if (one) { q.bias = p->b[l]; q.bias_mod = g.cout[l]; q.flags = l < 4 ? DM_GEMM_ELU : 0; }
      DM_TRY(dm_gemm_launch(q, splitk, skb, st));
      if (!one)
        DM_TRY(dm_col2im_s2_launch(n, g.hbg[l], g.hbg[l], g.cout[l], g.k[l], ycol, p->b[l], l < 4 ? DM_C2I_ELU : 0, nullptr,
                                   a.x[l], st));
    }
  }
  if (loss_image || image_rec) {
    // targets are indexed by frame / I (I = iwae_samples, decoders.py:163-167)
    const int I = shp->I > 0 ? shp->I : 1;
    DM_TRY(mse_launch(shape_u8(shp), n, g.hbg[4] * g.hbg[4], g.ch, a.x[4], target, I, 0.f, nullptr, loss_image, nullptr, g.ch,
                      image_rec, st));
  }
  return DM_OK;
}
// The backward's workspace.  One gradient buffer per layer (together smaller than a ping-pong pair of the largest) and one
// gather table pair per layer: a layer's weight / bias gradient only reads G[l], its tables and the saved activations, so those
// launches can sit on the weight-gradient side stream (common.h, dm_wgrad_side_*) and run beside whatever follows the
// DATA-gradient chain on `st` - the BPTT loop - instead of in front of it.  Every layer's output gradient is gathered
// implicitly: channel counts that are not a multiple of 4 (the 3-channel image layer) are padded to 4 (co4) in the gradient
// buffer and in a padded copy of the weights (wpad).  l4_*: the image layer's direct kernels.  On an arena without a base it sizes.
struct DecBwdWs {
  float *splitk, *splitk_w, *Gl[5], *dwr, *wpad, *bsum, *l4_wp, *l4_part;
  int *rowoff[5], *koff[5];      // index 1..4
  unsigned short *Gl_h[5], *wpad_h;
  int co4[5]; size_t gsz[5], wpadmax;
};
static size_t dec_bwd_layout(DmArena ar, const DecGeom& g, const ConvPlan& pl, bool tw_on, DecBwdWs* w) {
  const bool direct4 = pl.form[4] == CONV_DIRECT;
  w->splitk = ar.take(DM_SPLITK_FLOATS);
  size_t wmax = 0;
  w->co4[0] = 0; w->gsz[0] = (size_t)g.N * g.cin[1]; w->wpadmax = 0;
  for (int l = 1; l <= 4; ++l) {
    const int co = w->co4[l] = (g.cout[l] + 3) & ~3;
    w->gsz[l] = g.rows_b[l] * co;
    const size_t wl = (size_t)g.cin[l] * g.k[l] * g.k[l] * co;
    if (wl > wmax) wmax = wl;
    if (co != g.cout[l] && wl > w->wpadmax) w->wpadmax = wl;
  }
  for (int l = 0; l <= 4; ++l) w->Gl[l] = ar.take(w->gsz[l]);
  w->dwr = ar.take(wmax);
  w->wpad = ar.take(w->wpadmax);
  w->bsum = ar.take(64);
  w->rowoff[0] = w->koff[0] = nullptr;
  for (int l = 1; l <= 4; ++l) {
    w->rowoff[l] = (int*)ar.take(g.rows_s[l]);
    w->koff[l] = (int*)ar.take((size_t)g.k[l] * g.k[l] * w->co4[l]);
  }
  w->splitk_w = ar.take(DM_SPLITK_FLOATS);          // the side stream's own split-K scratch
  w->l4_wp = ar.take(direct4 ? dm_dec_l4_wp_floats(g.d) : 0);
  w->l4_part = ar.take(direct4 ? dm_dec_l4_wgrad_part_floats(g.N, g.d) : 0);
  // bf16 mode: twins of the gradient buffers and of the padded image-layer weights
  for (int l = 0; l <= 4; ++l) w->Gl_h[l] = (unsigned short*)ar.take(tw_on ? dm_half_floats(w->gsz[l]) : 0);
  w->wpad_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(w->wpadmax) : 0);
  return ar.off;
}
// sizing: the image layer's direct backward kernels wherever the shape admits them (a call also asks dm_dec_l4_bwd_direct_enable)
static ConvPlan dec_bwd_plan(const DecGeom& g, bool tw_on, bool sizing) {
  ConvPlan pl;
  const bool direct4 = sizing ? dec_direct4(g) : dm_dec_l4_bwd_direct_ok(g.ch, g.d, g.hsm[4], g.k[4]);
  for (int l = 4; l >= 1; --l) {
    pl.form[l] = l == 4 && direct4 ? CONV_DIRECT : CONV_IMPLICIT;
    if (g.cout[l] & 3) pl.bits[l] |= CONV_PADDED;      // the output gradient and a copy of the weights carry (cout + 3) & ~3 channels
    // the layer below gathers its output gradient at a padded pitch (cnn_depth 6: 6 -> 8): the data gradient is written at that pitch
    if (pl.form[l] == CONV_IMPLICIT && l >= 2 && (g.cout[l - 1] & 3)) pl.bits[l] |= CONV_REPITCH;
  }
  DecBwdWs w;
  pl.need = dec_bwd_layout(DmArena(nullptr, 0), g, pl, tw_on, &w);
  return pl;
}
// the bias gradient of a layer with padded channels: column sums of all co into bsum, the first cout of them to db
static int dec_bias_grad_padded(int rows, int co, const float* G, float* bsum, int cout, float* db, float* splitk, hipStream_t sw) {
  DM_TRY(dm_colsum_launch(rows, co, G, co, bsum, splitk, DM_SPLITK_FLOATS * sizeof(float), sw));
  hipError_t e = hipMemcpyAsync(db, bsum, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, sw);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "conv_decoder_bwd: %s", hipGetErrorString(e));
  return DM_OK;
}

static int conv_decoder_mse_bwd_impl(const dm_shape* shp, const float* feat, int ldf, const float* target,
                                     const dm_conv_params* p, const float* acts, float scale, const float* row_scale,
                                     const dm_conv_grads* gr, float* dfeat, int lddf, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(shp && feat && target && p && acts && gr && ws, DM_E_NULL, "conv_decoder_bwd: null pointer");
  DmPrecisionScope prec(shp->flags & DM_FLAG_BF16);
  DecGeom g(shp);
  DM_REQUIRE(g.valid(shp), DM_E_SHAPE, "conv_decoder: unsupported geometry");
  hipStream_t st = (hipStream_t)stream;
  DecActs a;
  dec_carve(g, const_cast<float*>(acts), (size_t)1 << 60, &a);
  DmTwinScope tw((shp->flags & DM_FLAG_BF16) != 0);
  const bool tw_on = dm_twins_on();
  const ConvPlan pl = dec_bwd_plan(g, tw_on, false);
  DecBwdWs w;
  dec_bwd_layout(DmArena(ws, ws_bytes), g, pl, tw_on, &w);
  DM_REQUIRE(pl.need <= ws_bytes / sizeof(float), DM_E_WORKSPACE, "conv_decoder_bwd: workspace too small (need %zu floats)", pl.need);
  const auto& [splitk, splitk_w, Gl, dwr, wpad, bsum, l4_wp, l4_part, rowoff_l, koff_l, Gl_h, wpad_h, co4, gsz, wpadmax] = w;
  const size_t skb = DM_SPLITK_FLOATS * sizeof(float);
  const bool arena_tw = dm_twin_arena_valid(acts);      // the forward that filled `acts` wrote its twins
  dec_register_twins(g, a, arena_tw, arena_tw);
  for (int l = 0; l <= 4; ++l)
    if (pl.form[l] != CONV_DIRECT) dm_twin_add(Gl[l], gsz[l], Gl_h[l], false);      // (the direct kernels read the fp32 gradient)
  dm_twin_add(wpad, wpadmax, wpad_h, false);
  hipStream_t sw = dm_wgrad_side_stream(st);

  // G4 = scale * (pred - target), NHWC with co4[4] channels per pixel
  float* G = Gl[4];
  DM_TRY(mse_launch(shape_u8(shp), g.N, g.hbg[4] * g.hbg[4], g.ch, a.x[4], (const void*)target, shp->I > 0 ? shp->I : 1, scale,
                    row_scale, nullptr, G, co4[4], nullptr, st));
  for (int l = 4; l >= 1; --l) {
    const int kk = g.k[l] * g.k[l], co = co4[l], ncol = kk * co, rows_s = (int)g.rows_s[l];
    const bool padded = pl.bits[l] & CONV_PADDED;
    int *rowoff = rowoff_l[l], *koff = koff_l[l];
    float* Gn = Gl[l - 1];
    if (pl.form[l] == CONV_DIRECT) {
      DM_TRY(dm_wgrad_side_fork(st, sw));
      unsigned short* gnh = dm_twin_of(Gn, false);
      DM_TRY(dm_dec_l4_dgrad_launch(g.N, g.d, G, p->w[4], l4_wp, a.x[3], Gn, gnh, st));
      if (gnh) dm_twin_mark(Gn);
      DM_TRY(dec_bias_grad_padded((int)g.rows_b[l], co, G, bsum, g.cout[l], gr->b[l], splitk_w, sw));
      DM_TRY(dm_dec_l4_wgrad_launch(g.N, g.d, G, a.x[3], l4_part, gr->w[4], splitk_w, skb, sw));
      G = Gn;
      continue;
    }
    // patches of the output gradient, gathered implicitly (16-byte gathers: co is a multiple of 4)
    DM_TRY(conv_tables_launch(g.N, g.hbg[l], g.hbg[l], co, g.k[l], rowoff, koff, st));
    DM_TRY(dm_wgrad_side_fork(st, sw));                  // G[l] and its tables are enqueued: the side stream may read them
    // ---- data gradient (the chain the BPTT loop waits for), on st
    if (padded) {
      hipLaunchKernelGGL(convt_pad_cout_kernel, dim3(grid_for((size_t)g.cin[l] * ncol)), dim3(256), 0, st, g.cin[l], g.cout[l], co,
                         g.k[l], p->w[l], wpad);
      DM_LAUNCH_CHECK();
      if (tw_on) {
        const DmCvtSeg sg = {wpad, wpad_h, (size_t)g.cin[l] * ncol};
        DM_TRY(dm_to_bf16_multi_launch(&sg, 1, st));
        dm_twin_mark(wpad);
      }
    }
    {
      DmGemm d;   // dX[row][i] = sum_col dYcol[row][col] * Wr[i][col]   (* ELU'(X_{l-1}) for l-1 >= 1)
      d.a_layout = 0; d.b_layout = 0;
      d.M = rows_s; d.N = g.cin[l]; d.K = ncol;
      d.A = G; d.a_maj = rowoff; d.a_min = koff; d.a_tab_vec = 1;
      d.a_tab_vec8 = (co & 7) == 0 || (co == 4 && (g.k[l] & 1) == 0);
      d.B = padded ? wpad : a.wr[l]; d.ldb = ncol;
      d.C = Gn; d.ldc = g.cin[l];
      if (pl.bits[l] & CONV_REPITCH) {      // rows at the pitch co4[l-1] of the layer below, over zeroed pad channels
        hipError_t e = hipMemsetAsync(Gn, 0, gsz[l - 1] * sizeof(float), st);
        if (e == hipSuccess && dm_twin_of(Gn, false))
          e = hipMemsetAsync(dm_twin_of(Gn, false), 0, gsz[l - 1] * sizeof(unsigned short), st);
        if (e != hipSuccess) return dm_fail(DM_E_HIP, "conv_decoder_bwd: %s", hipGetErrorString(e));
        d.ldc = co4[l - 1];
      }
      if (l - 1 >= 1) { d.mulref = a.x[l - 1]; d.ldmul = g.cin[l]; }
      DM_TRY(dm_gemm_launch(d, splitk, skb, st));
    }
    // ---- bias and weight gradient, on sw
    if (padded) DM_TRY(dec_bias_grad_padded((int)g.rows_b[l], co, G, bsum, g.cout[l], gr->b[l], splitk_w, sw));
    else DM_TRY(dm_colsum_launch((int)g.rows_b[l], co, G, co, gr->b[l], splitk_w, skb, sw));
    DmGemm q;   // dWr[i][(ky,kx,o)] = sum_rows X[row][i] * dYcol[row][(ky,kx,o)]
    q.a_layout = 1; q.b_layout = 1;
    q.M = g.cin[l]; q.N = ncol; q.K = rows_s;
    q.A = a.x[l - 1]; q.lda = g.cin[l];
    q.B = G; q.b_maj = rowoff; q.b_min = koff; q.b_tab_vec = 1;
    q.b_tab_vec8 = (co & 7) == 0 || (co == 4 && (g.k[l] & 1) == 0);      // 8 minors = 8 channels, or 2 pixels x 4 channels of an even-width window
    q.C = dwr; q.ldc = ncol;
    DM_TRY(dm_gemm_launch(q, splitk_w, skb, sw));
    if (padded) {
      hipLaunchKernelGGL(convt_unpad_cout_kernel, dim3(grid_for((size_t)g.cin[l] * kk * g.cout[l])), dim3(256), 0, sw, g.cin[l],
                         g.cout[l], co, g.k[l], dwr, gr->w[l]);
      DM_LAUNCH_CHECK();
    } else {
      DM_TRY(dm_permute4_launch(dwr, gr->w[l], g.cin[l], g.k[l], g.k[l], g.cout[l], 0, 3, 1, 2, sw));
    }
    G = Gn;
  }
  // fc: x0 = feat W^T + b
  const int O = g.cin[1];
  DM_TRY(dm_wgrad_side_fork(st, sw));
  if (dfeat) {
    DmGemm d;   // dfeat[n][f] += sum_o G[n][o] W[o][f]
    d.a_layout = 0; d.b_layout = 1;
    d.M = g.N; d.N = g.F; d.K = O;
    d.A = G; d.lda = O;
    d.B = p->w[0]; d.ldb = g.F;
    d.C = dfeat; d.ldc = lddf;
    d.flags = DM_GEMM_ACCUM;
    DM_TRY(dm_gemm_launch(d, splitk, skb, st));
  }
  DM_TRY(dm_colsum_launch(g.N, O, G, O, gr->b[0], splitk_w, skb, sw));
  {
    DmGemm q;   // dW[o][f] = sum_n G[n][o] feat[n][f]
    q.a_layout = 1; q.b_layout = 1;
    q.M = O; q.N = g.F; q.K = g.N;
    q.A = G; q.lda = O;
    q.B = feat; q.ldb = ldf;
    q.C = gr->w[0]; q.ldc = g.F;
    DM_TRY(dm_gemm_launch(q, splitk_w, skb, sw));
  }
  DM_TRY(dm_wgrad_side_mark(sw, st));
  return DM_OK;
}
extern "C" int dm_conv_decoder_mse_bwd(const dm_shape* shp, const float* feat, int ldf, const float* target,
                                       const dm_conv_params* p, const float* acts, float scale, const dm_conv_grads* gr,
                                       float* dfeat, int lddf, void* ws, size_t ws_bytes, void* stream) {
  return conv_decoder_mse_bwd_impl(shp, feat, ldf, target, p, acts, scale, nullptr, gr, dfeat, lddf, ws, ws_bytes, stream);
}
// row_scale (N floats, nullable): per-frame factor on the image-loss gradient - the IWAE importance weights of
// loss_model = -logavgexp(-loss_tbi) (dreamer.py:362-365, functions.py:97-102)
extern "C" int dm_conv_decoder_mse_bwd_rows(const dm_shape* shp, const float* feat, int ldf, const float* target,
                                            const dm_conv_params* p, const float* acts, float scale, const float* row_scale,
                                            const dm_conv_grads* gr, float* dfeat, int lddf, void* ws, size_t ws_bytes,
                                            void* stream) {
  return conv_decoder_mse_bwd_impl(shp, feat, ldf, target, p, acts, scale, row_scale, gr, dfeat, lddf, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- workspace sizing (common.h) ----
// DM_FLAG_BF16 sizes the twins whatever dm_bf16_twins_enable says; reward_input and the direct image-layer backward are sized
// wherever the shape admits them.
size_t dm_conv_ws_floats(const dm_shape* s, size_t parts[4]) {
  size_t p[4] = {0, 0, 0, 0};
  const bool geom = s && s->T >= 0 && s->B >= 0 && s->img == 64 && s->img_ch >= 1 && s->cnn_depth >= 1;      // (else the geometry structs would wrap)
  if (geom) {
    const bool tw = (s->flags & DM_FLAG_BF16) != 0;
    const EncGeom e(s); const DecGeom d(s);
    if (e.valid(s) || e.valid_planes(s)) { p[0] = enc_fwd_plan(e, e.valid_planes(s)).need; p[1] = enc_bwd_plan(e, e.valid_planes(s), tw).need; }
    if (d.valid(s)) { p[2] = dec_fwd_plan(d, tw).need; p[3] = dec_bwd_plan(d, tw, true).need; }
  }
  for (int i = 0; i < 4 && parts; ++i) parts[i] = p[i];
  return std::max(std::max(p[0], p[1]), std::max(p[2], p[3]));
}

// include/dreamer_hip.h dm_conv_plan_query: the plan a call of entry point `which` would carry out, the switches as they stand
extern "C" int dm_conv_plan_query(int which, const dm_shape* shp, int planes, int32_t out[8], size_t* need_floats) {
  DM_REQUIRE(shp && out, DM_E_NULL, "conv_plan_query: null pointer");
  DM_REQUIRE((unsigned)which <= 3 && shp->T >= 0 && shp->B >= 0 && shp->img_ch >= 1 && shp->cnn_depth >= 1, DM_E_SHAPE,
             "conv_plan_query: which %d, T=%d B=%d ch=%d depth=%d", which, shp->T, shp->B, shp->img_ch, shp->cnn_depth);
  const bool tw_on = (shp->flags & DM_FLAG_BF16) && dm_bf16_twins_enable(-1);
  const EncGeom e(shp); const DecGeom d(shp);
  if (which <= 1) DM_TRY(enc_validate(shp, e, planes != 0, 32 * e.d, "conv_plan_query"));
  else DM_REQUIRE(d.valid(shp), DM_E_SHAPE, "conv_plan_query: unsupported decoder geometry (img=%d)", shp->img);
  const ConvPlan pl = which == 0 ? enc_fwd_plan(e, planes != 0) : which == 1 ? enc_bwd_plan(e, planes != 0, tw_on)
                    : which == 2 ? dec_fwd_plan(d, tw_on) : dec_bwd_plan(d, tw_on, false);
  for (int l = 0; l < 5; ++l) out[l] = pl.form[l] < 0 ? -1 : pl.form[l] | pl.bits[l] << 8;
  out[5] = pl.kskip; out[6] = out[7] = 0;
  if (need_floats) *need_floats = pl.need;
  return DM_OK;
}
