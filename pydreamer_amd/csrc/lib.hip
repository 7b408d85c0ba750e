// Library-level entry points: version, error string, device check, workspace sizing.
#include "common.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>

static thread_local char g_err[512] = "";

int dm_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" int dm_version(void) { return 17; }
extern "C" const char* dm_last_error(void) { return g_err; }

extern "C" int dm_device_check(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return dm_fail(DM_E_DEVICE, "hipGetDevice failed (no HIP device visible)");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return dm_fail(DM_E_DEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return dm_fail(DM_E_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
  return DM_OK;
}

// A HIP stream restricted to a subset of the compute units (hipExtStreamCreateWithCUMask): `mask` has one bit per CU, 32
// per word.  bench.py's DM_MAIN_RESERVE_CUS experiment runs the caller's stream on one.
extern "C" int dm_stream_create_cu_mask(const uint32_t* mask, int words, void** stream) {
  DM_REQUIRE(mask && stream && words >= 1, DM_E_NULL, "stream_create_cu_mask: null argument");
  hipStream_t s = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "hipExtStreamCreateWithCUMask: %s", hipGetErrorString(e));
  *stream = (void*)s;
  return DM_OK;
}
extern "C" int dm_stream_destroy(void* stream) {
  if (!stream) return DM_OK;
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "hipStreamDestroy: %s", hipGetErrorString(e));
  return DM_OK;
}

// ---- weight-gradient side stream (see include/dreamer_hip.h) ---------------------------------------------------------
// One stream + two events per process (one process drives one GPU); the armed flag is per host thread, because the
// world-model backward is enqueued by one thread while others enqueue the rollout / actor-critic passes.
static std::mutex g_side_mu;
static hipStream_t g_side_stream = nullptr;
static hipEvent_t g_side_fork_ev[8] = {nullptr}, g_side_done_ev = nullptr;      // fork events rotate: one per fork point in flight
static unsigned g_side_fork_i = 0;
static int g_side_dev = -1;
static bool g_side_pending = false;
static thread_local bool tl_side_armed = false;

static int side_init_locked() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return dm_fail(DM_E_DEVICE, "wgrad_side: hipGetDevice failed");
  if (g_side_stream && dev == g_side_dev) return DM_OK;
  if (g_side_stream) return dm_fail(DM_E_DEVICE, "wgrad_side: created on device %d, called on device %d", g_side_dev, dev);
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  // lowest priority: the chains' small kernels dispatch first
  hipError_t e = hipStreamCreateWithPriority(&g_side_stream, hipStreamNonBlocking, least);
  for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&g_side_fork_ev[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&g_side_done_ev, hipEventDisableTiming);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "wgrad_side: %s", hipGetErrorString(e));
  g_side_dev = dev;
  return DM_OK;
}

extern "C" int dm_wgrad_side_arm(int on) {
  if (on) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    DM_TRY(side_init_locked());
  }
  tl_side_armed = on != 0;
  return DM_OK;
}

// Creates the side stream NOW and gives it one command, so that it holds its hardware queue before anything else (a communicator's
// internal streams, torch's communication stream) asks for one: round 6 measured that the order in which streams first get work
// decides which of them end up sharing a hardware queue (profiles/r06_force_dp.txt, runs C / G / H).
extern "C" int dm_wgrad_side_touch(void) {
  std::lock_guard<std::mutex> lk(g_side_mu);
  DM_TRY(side_init_locked());
  static float* pad = nullptr;
  if (!pad && hipMalloc(reinterpret_cast<void**>(&pad), 256) != hipSuccess) return dm_fail(DM_E_HIP, "wgrad_side_touch: hipMalloc failed");
  if (hipMemsetAsync(pad, 0, 256, g_side_stream) != hipSuccess) return dm_fail(DM_E_HIP, "wgrad_side_touch: memset failed");
  return DM_OK;
}

hipStream_t dm_wgrad_side_stream(hipStream_t st) { return tl_side_armed && g_side_stream ? g_side_stream : st; }

int dm_wgrad_side_fork(hipStream_t st, hipStream_t sw) {
  if (sw == st) return DM_OK;
  std::lock_guard<std::mutex> lk(g_side_mu);
  hipEvent_t ev = g_side_fork_ev[g_side_fork_i++ & 7];
  hipError_t e = hipEventRecord(ev, st);
  if (e == hipSuccess) e = hipStreamWaitEvent(sw, ev, 0);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "wgrad_side fork: %s", hipGetErrorString(e));
  return DM_OK;
}

int dm_wgrad_side_mark(hipStream_t sw, hipStream_t st) {
  if (sw == st) return DM_OK;
  std::lock_guard<std::mutex> lk(g_side_mu);
  hipError_t e = hipEventRecord(g_side_done_ev, sw);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "wgrad_side mark: %s", hipGetErrorString(e));
  g_side_pending = true;
  return DM_OK;
}

extern "C" int dm_wgrad_side_join(void* stream) {
  tl_side_armed = false;
  std::lock_guard<std::mutex> lk(g_side_mu);
  if (!g_side_pending) return DM_OK;
  hipError_t e = hipStreamWaitEvent((hipStream_t)stream, g_side_done_ev, 0);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "wgrad_side join: %s", hipGetErrorString(e));
  g_side_pending = false;
  return DM_OK;
}

// Scratch sizing: every fused operator carves its workspace with a layout function of its own (conv.hip, rssm.hip, mlp.hip);
// the same functions, run on an arena without a base, say what each needs (common.h dm_*_ws_floats).  The caller's buffer
// serves them one at a time: the largest, plus a slack of 4096 floats.  See DESIGN.md "HBM layout".
extern "C" int dm_workspace_query(const dm_shape* s, size_t* parts, int n) {
  DM_REQUIRE(s && parts && n >= 8, DM_E_NULL, "workspace_query: null argument, or room for fewer than 8 parts");
  dm_conv_ws_floats(s, parts);
  dm_rssm_ws_floats(s, parts + 4);
  parts[6] = dm_rollout_ws_floats(s);
  const long long rows = (long long)(s->H > 0 ? s->H + 1 : 2) * s->T * s->B * (s->I > 0 ? s->I : 1);      // the heads' rows: every imagined step of every row
  parts[7] = dm_mlp_ws_floats((int)rows, s->mlp_hidden, s->mlp_layers);
  return DM_OK;
}
extern "C" size_t dm_workspace_bytes(const dm_shape* s) {
  size_t parts[8], m = 0;
  if (dm_workspace_query(s, parts, 8) != DM_OK) return 0;
  for (size_t v : parts) m = v > m ? v : m;
  return (m + 4096) * sizeof(float);
}
