// Device-resident replay (pydreamer_amd/replay.py DeviceReplay): one launch assembles a (T, B, ...) batch of every field out of
// episodes that live in HBM.  A batch column b is one or two pieces (start row, length, mark) of one or two episodes (the
// planner's windows, SequentialReplay._plan); destination row t*B + b of every field is row start + t' of the piece that holds t.
//
// One workgroup per destination row (grid-strided).  Everything that selects the source - the column's piece, its row, the
// source base of each field - depends on blockIdx alone, so it is decoded once per workgroup in scalar registers; the lanes
// only stride over the row's bytes.  The frame field (64 x 64 x 3 uint8 = 12 288 B per row, ~all of the bytes) moves as 16 B
// per lane, consecutive lanes on consecutive chunks: 768 chunks = three 256-lane sweeps, issued as independent loads before
// the first store.  The small fields (one-hot actions, reward, terminal, reset, vecobs, map fields) ride in the same launch at
// the widest access their row size allows.
#include "common.h"

namespace {

struct GatherFields {
  dm_replay_field f[DM_REPLAY_MAX_FIELDS];
};

constexpr int kThreads = 256;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define DM_GLOBAL __attribute__((address_space(1)))      // the source bases are loaded from a table: tell the compiler they are global

// n units of V from s to d, consecutive lanes on consecutive units; four independent loads in flight per lane before the first store
template <typename V>
__device__ __forceinline__ void copy_units(const DM_GLOBAL V* __restrict__ s, DM_GLOBAL V* __restrict__ d, unsigned n) {
  for (unsigned i0 = threadIdx.x; i0 < n; i0 += kThreads * 4) {
    const unsigned i1 = i0 + kThreads, i2 = i0 + 2 * kThreads, i3 = i0 + 3 * kThreads;
    V v0 = s[i0], v1, v2, v3;
    if (i1 < n) v1 = s[i1];
    if (i2 < n) v2 = s[i2];
    if (i3 < n) v3 = s[i3];
    d[i0] = v0;
    if (i1 < n) d[i1] = v1;
    if (i2 < n) d[i2] = v2;
    if (i3 < n) d[i3] = v3;
  }
}

// pieces (B, 2, 3): start row, length, mark;  src (B, 2, nf): base of the field in the piece's episode
__global__ void __launch_bounds__(kThreads) replay_gather_kernel(GatherFields a, int nf, int B, long long rows,
                                                                 const int32_t* __restrict__ pieces,
                                                                 const uintptr_t* __restrict__ src) {
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int t = (int)(row / B), b = (int)(row - (long long)t * B);
    const int32_t* pc = pieces + (size_t)b * 6;
    const int len0 = pc[1];
    const int p = t >= len0 ? 1 : 0;
    const int tl = p ? t - len0 : t;                          // row inside the piece
    const size_t srow = (size_t)pc[3 * p] + (size_t)tl;
    const bool marked = pc[3 * p + 2] != 0 && tl == 0;        // an artificial reset lands on the piece's first row
    const uintptr_t* sp = src + ((size_t)b * 2 + p) * nf;
    for (int f = 0; f < nf; ++f) {
      const size_t rb = (size_t)a.f[f].row_bytes;
      const uintptr_t s = sp[f] + srow * rb;
      const uintptr_t d = (uintptr_t)a.f[f].dst + (size_t)row * rb;
      if ((rb & 15) == 0) {
        copy_units((const DM_GLOBAL u32x4*)s, (DM_GLOBAL u32x4*)d, (unsigned)(rb >> 4));
      } else if ((rb & 3) == 0) {
        copy_units((const DM_GLOBAL uint32_t*)s, (DM_GLOBAL uint32_t*)d, (unsigned)(rb >> 2));
      } else if (a.f[f].is_reset && marked) {
        if (threadIdx.x == 0) *(DM_GLOBAL uint8_t*)d = 1;     // row_bytes == 1 (checked on the host)
      } else {
        copy_units((const DM_GLOBAL uint8_t*)s, (DM_GLOBAL uint8_t*)d, (unsigned)rb);
      }
    }
  }
}

}  // namespace

extern "C" int dm_replay_gather(int T, int B, int nfields, const dm_replay_field* fields, const int32_t* pieces,
                                const void* const* src, void* stream) {
  DM_REQUIRE(fields && pieces && src, DM_E_NULL, "replay_gather: null pointer (fields / pieces / src)");
  DM_REQUIRE(T >= 1 && B >= 1, DM_E_SHAPE, "replay_gather: bad shape T=%d B=%d", T, B);
  DM_REQUIRE(nfields >= 1 && nfields <= DM_REPLAY_MAX_FIELDS, DM_E_SHAPE, "replay_gather: %d fields, 1..%d supported", nfields,
             DM_REPLAY_MAX_FIELDS);
  DM_REQUIRE(((uintptr_t)pieces & 3) == 0 && ((uintptr_t)src & 7) == 0, DM_E_SHAPE,
             "replay_gather: the piece table must be 4-byte and the source table 8-byte aligned");
  GatherFields a;
  int resets = 0;
  for (int f = 0; f < nfields; ++f) {
    const dm_replay_field& q = fields[f];
    DM_REQUIRE(q.dst, DM_E_NULL, "replay_gather: field %d has a null destination", f);
    DM_REQUIRE(((uintptr_t)q.dst & 15) == 0, DM_E_SHAPE, "replay_gather: field %d: the destination must be 16-byte aligned", f);
    DM_REQUIRE(q.row_bytes >= 1 && q.row_bytes <= ((int64_t)1 << 31), DM_E_SHAPE, "replay_gather: field %d: %lld bytes per row", f,
               (long long)q.row_bytes);
    if (q.is_reset) {
      DM_REQUIRE(q.row_bytes == 1, DM_E_SHAPE, "replay_gather: the reset column is one byte per row, field %d has %lld", f,
                 (long long)q.row_bytes);
      ++resets;
    }
    a.f[f] = q;
  }
  DM_REQUIRE(resets <= 1, DM_E_SHAPE, "replay_gather: %d fields are flagged as the reset column", resets);
  for (int f = nfields; f < DM_REPLAY_MAX_FIELDS; ++f) a.f[f] = dm_replay_field{nullptr, 0, 0, 0};
  const long long rows = (long long)T * B;
  const unsigned grid = (unsigned)(rows < (1 << 20) ? rows : (1 << 20));
  hipLaunchKernelGGL(replay_gather_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a, nfields, B, rows, pieces,
                     (const uintptr_t*)src);
  DM_LAUNCH_CHECK();
  return DM_OK;
}
