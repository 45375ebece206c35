// Internals shared by the engine's translation units (engine.cpp: life cycle, workspaces, graphs, the synthesis call;
// engine_stream.cpp: the one-utterance stream, the batch stream, the pool, the stream gain; engine_deliver.cpp: what lies
// behind the generator -- output rate, target loudness, true peak, limiter -- with its filters, setters, buffers and hooks;
// engine_pack.cpp: voice -> packed weight arena; engine_launch.cpp: one launcher per kernel family; engine_issue.cpp: the
// kernel sequence of the pipeline stages). Not part of any interface.
#pragma once
#include "engine.h"
#include "kernels/launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <shared_mutex>

namespace pe {

// a launch with a level-2 profile row of its own (the element-wise / integer glue kernels; the conv / attention /
// fused-stage launchers bracket themselves and also carry FLOP and byte counts)
#define PE_LAUNCH_KB(kname, bytes, call)                                         \
  do {                                                                           \
    const int kh_ = kbegin(prof_level_ >= 2 ? krow(kname) : 0, 0.0, (bytes));    \
    call;                                                                        \
    kend(kh_);                                                                   \
  } while (0)
#define PE_LAUNCH_K(kname, call) PE_LAUNCH_KB(kname, 0.0, call)

// Engines that share a process (pe_group_*: one per device, each on its own thread) must not be inside a HIP call while
// another one CAPTURES a graph: allocations / synchronising copies on a second thread invalidate a capture in progress on
// this runtime, whatever the capture mode. Every public entry holds this lock shared; a capture takes it exclusively.
// A single engine per process never contends. (Defined in engine.cpp.)
extern std::shared_mutex g_capture_mu;
extern thread_local int g_entry_depth;
struct EntryLock {
  EntryLock() { if (g_entry_depth++ == 0) g_capture_mu.lock_shared(); }
  ~EntryLock() { if (--g_entry_depth == 0) g_capture_mu.unlock_shared(); }
};

static inline int rup(int v, int m) { return (v + m - 1) / m * m; }

// PIPER_HIP_DEBUG_POISON: a freshly allocated workspace is filled with NaN bit patterns so that a kernel relying on memory
// it never wrote shows up in the result. The fill runs on the null stream and is asynchronous to the host, while the
// engine's stream does not synchronise with the null stream: without the wait below the fill could land AFTER the first
// copies / launches into the new buffer (seen as NaNs in the first injected noise row, profiles/r05_notes.md, call 31-35).
static inline void poison(void* p, size_t bytes) {
  PE_HIP(hipMemset(p, 0xFF, bytes));
  PE_HIP(hipDeviceSynchronize());
}

template <class Buf>
void Engine::side_alloc(Buf& b, size_t n, bool idle, Fill fill, const char* what, size_t what_bytes) {
  if (idle) {
    PE_HIP(hipStreamSynchronize(stream_));
    if (b) drop_graphs();
  }
  b.reset();
  b.grow(n, what, what_bytes);
  if (fill == FILL_ZERO || (fill == FILL_POISON_OR_ZERO && !pol_.debug_poison)) b.zero();
  else if (fill != FILL_NONE && pol_.debug_poison) poison(b.get(), b.bytes());
}

// A pinned host buffer of at least n elements: grown with half as much again on top, its content not kept.
template <typename T>
static inline void grow_pinned(PinBuf<T>& b, size_t n) {
  if (n > b.size()) b.grow(n + n / 2);
}

template <typename T>
void Engine::rows_to_device(T* dst, long xs, const T* src, int batch, int64_t stride) {
  for (int b = 0; b < batch && stride > 0; ++b)
    PE_HIP(hipMemcpyAsync(dst + (size_t)b * xs, src + (size_t)b * stride, (size_t)stride * sizeof(T), hipMemcpyHostToDevice, stream_));
}
template <typename T>
void Engine::rows_to_host(T* dst, int64_t stride, const T* src, long xs, int batch, const int32_t* count) {
  for (int b = 0; b < batch; ++b) {
    const size_t n = count ? (size_t)count[b] : (size_t)stride;
    if (n > 0) PE_HIP(hipMemcpyAsync(dst + (size_t)b * stride, src + (size_t)b * xs, n * sizeof(T), hipMemcpyDeviceToHost, stream_));
  }
}

// tile configurations of conv_mfma_kernel: {WM, WN, MT, NT}
enum { CFG_A = 0, CFG_B = 1, CFG_C = 2, CFG_S = 3, CFG_G = 4, CFG_C2 = 5, CFG_B2 = 6 };
static const int CFG_BM[] = {128, 64, 32, 64, 128, 32, 64};
static const int CFG_BN[] = {128, 128, 128, 64, 64, 256, 256};

// Workgroups of a launch on BM x BN tiles over `ncols` columns, `row_tiles` packed 32-row tiles and B utterances: the count
// every policy threshold is asked with.
static inline long tile_workgroups(int BM, int BN, int ncols, int row_tiles, int B) {
  return (long)((ncols + BN - 1) / BN) * (row_tiles * 32 / BM) * B;
}

// One conv launch, decided once by Engine::plan_conv and carried out by Engine::conv (or recorded into the open group).
enum ConvForm { CONV_TILE, CONV_SPLIT, CONV_1X1, CONV_SPLITK, CONV_SPLITK16, CONV_GATE12 };
struct ConvPlan {
  ConvForm form = CONV_TILE;  // tiled, split-operand tiled, one-tap direct, split-K, 16-column split-K, 12-column gate
  int ncols = 0;              // grid bound in columns (one more for a ConvTranspose)
  long blocks = 0;            // tile workgroups of the PACKED configuration: what the split-K / grouping thresholds were asked with
  int cfg = 0, halo = 64;     // launched tile configuration (CFG_*; split-operand: 0 / 1 / 2) and x-slab halo (64 / 128)
  int nw = 0, MT = 1, tgroups = 1, tpb = 1, nbuf = 2, up_vec = 0;      // split-K waves and row tiles per wave; ConvP fields
  bool half = false;          // 16-column gate form on half a channel group per workgroup
  dim3 grid;
  size_t smem = 0;
  bool group_splitk = false, group_tiled = false;      // may ride in a grouped split-K / grouped tiled launch ...
  int group_cfg = CFG_S;                               // ... the latter on this tile configuration (CFG_C or CFG_S)
};

// One coupling layer of a call, decided once by Engine::plan_flow and carried out by issue_flow's loop and the launch
// helpers wn_res_skip4 / coupling_chain.
struct FlowLayerPlan {
  bool chain = false;               // post + "x1 -= m" (+ the next layer's pre) as a chain launch, not conv(post)
  bool pre_launch = false;          // this layer's pre is a launch of its own (else: the previous chain wrote it, or it is composed) ...
  bool pre_col4 = false;            // ... on colchain4_kernel mode 3 through pre4pad, not conv()
  bool rs_front = false;            // the last res/skip conv rides in front of the chain launch
  bool compose_pre = false;         // pre composed into the first gate conv (gate4pre_kernel); the first res/skip launch writes h whole
  bool compose_post = false;        // post composed into the skip rows; the chain launch has no post GEMM
  bool chain_has_next_pre = false;  // the chain launch writes the next layer's hidden state
  std::vector<bool> rs_col4;        // per WN layer: its res/skip launch goes to colchain4_kernel mode 2, not conv()
};

}  // namespace pe
