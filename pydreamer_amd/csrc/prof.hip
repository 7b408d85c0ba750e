// Optional per-launch timing (HIP events on the launch stream), used by bench.py for the roofline line and by the tests that
// pin a product to the kernel that answered it (tests/gemm_pin.py).  Recorded by dm_gemm_launch (gemm.hip), the row-panel
// kernels (panel.hip) and the whole-MLP kernel (mlp_chain.hip) through dm_prof_slot_begin / _shape / _end (common.h).
// Profiling kinds: tile * 4 + a_layout * 2 + b_layout for the GEMM tile kernels (0..19; tile 0: 128x128, 1: 128x64, 2: 64x64,
// 3: 128x96, 4: 96x128), + 24 when the launch took gemm_dma_kernel; 20 = row-panel forward, 21 = row-panel backward,
// 22 = whole-MLP kernel.
#include "common.h"
#include <vector>

struct GemmProf {
  bool on = false;
  size_t cap = 0, n = 0;
  std::vector<hipEvent_t> ev;      // 2 per slot
  std::vector<long long> shape;    // 5 per slot: M, N, K, split count, gather/scatter flags (bench.py --shape-table)
  std::vector<double> flops, bytes;
  std::vector<int> kind;
};
static GemmProf g_prof;
static int prof_before(int kind, double flops, double bytes, hipStream_t st) {
  if (!g_prof.on || g_prof.n >= g_prof.cap) return -1;
  const int slot = (int)g_prof.n++;
  g_prof.flops[slot] = flops;
  g_prof.bytes[slot] = bytes;
  g_prof.kind[slot] = kind;
  (void)hipEventRecord(g_prof.ev[2 * slot], st);
  return slot;
}
static void prof_after(int slot, hipStream_t st) {
  if (slot >= 0) (void)hipEventRecord(g_prof.ev[2 * slot + 1], st);
}
bool dm_prof_active() { return g_prof.on; }
int dm_prof_slot_begin(int kind, double flops, double bytes, hipStream_t st) { return prof_before(kind, flops, bytes, st); }
void dm_prof_slot_end(int slot, hipStream_t st) { prof_after(slot, st); }
void dm_prof_slot_shape(int slot, int M, int N, int K, int nsplit, int flags) {
  if (slot < 0) return;
  long long* sh = &g_prof.shape[5 * (size_t)slot];
  sh[0] = M; sh[1] = N; sh[2] = K; sh[3] = nsplit; sh[4] = flags;
}
extern "C" int dm_prof_begin(int max_launches) {
  DM_REQUIRE(max_launches > 0 && max_launches <= (1 << 20), DM_E_SHAPE, "prof_begin: max_launches %d", max_launches);
  if ((size_t)max_launches > g_prof.ev.size() / 2) {
    const size_t have = g_prof.ev.size();
    g_prof.ev.resize(2 * (size_t)max_launches);
    for (size_t i = have; i < g_prof.ev.size(); ++i)
      if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return dm_fail(DM_E_HIP, "prof_begin: hipEventCreate failed");
  }
  g_prof.flops.assign(max_launches, 0.0);
  g_prof.bytes.assign(max_launches, 0.0);
  g_prof.kind.assign(max_launches, 0);
  g_prof.shape.assign(5 * (size_t)max_launches, 0);
  g_prof.cap = max_launches;
  g_prof.n = 0;
  g_prof.on = true;
  return DM_OK;
}
// Per-launch rows of the profiled region, BEFORE dm_prof_end: rows[i*8 + {0..7}] = {kind, M, N, K, split count, flags
// (1 gathered A, 2 gathered B, 4 scatter epilogue, 8 bf16 operands), flops, milliseconds}; M = 0 for the non-GEMM kinds
// (row panels, whole-MLP kernel).  Returns the number of rows written (<= max_rows).  Synchronises on the events.
extern "C" int dm_prof_rows(double* rows, int max_rows) {
  DM_REQUIRE(rows && max_rows > 0, DM_E_NULL, "prof_rows: null output");
  int n = 0;
  for (size_t i = 0; i < g_prof.n && n < max_rows; ++i, ++n) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return dm_fail(DM_E_HIP, "prof_rows: event sync failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess)
      return dm_fail(DM_E_HIP, "prof_rows: hipEventElapsedTime failed");
    double* r = rows + 8 * (size_t)n;
    r[0] = g_prof.kind[i];
    for (int j = 0; j < 5; ++j) r[1 + j] = (double)g_prof.shape[5 * i + j];
    r[6] = g_prof.flops[i]; r[7] = ms;
  }
  return n;
}
// out[kind*4 + {0,1,2,3}] = {launches, flops, milliseconds, algorithmic bytes (4*(M*K + N*K + M*N))} for
// kind = tile*4 + a_layout*2 + b_layout (tile 0: 128x128, 1: 128x64, 2: 64x64, 3: 128x96, 4: 96x128), + 24 when the launch took
// gemm_dma_kernel; 20..22 panel / whole-MLP kernels; returns the number of recorded launches
// (negative on error).  Synchronises on the recorded events.
extern "C" int dm_prof_end(double* out, int nkinds) {
  DM_REQUIRE(out && nkinds >= 44, DM_E_SHAPE, "prof_end: need room for 44 kinds");
  g_prof.on = false;
  for (int i = 0; i < nkinds * 4; ++i) out[i] = 0.0;
  for (size_t i = 0; i < g_prof.n; ++i) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return dm_fail(DM_E_HIP, "prof_end: event sync failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess)
      return dm_fail(DM_E_HIP, "prof_end: hipEventElapsedTime failed");
    const int k = g_prof.kind[i];
    out[k * 4 + 0] += 1.0;
    out[k * 4 + 1] += g_prof.flops[i];
    out[k * 4 + 2] += ms;
    out[k * 4 + 3] += g_prof.bytes[i];
  }
  return (int)g_prof.n;
}
