// Native tree-grow driver: runs the entire per-tree level loop in C++
// so the only Python work per tree is gradient computation and cache
// update.  (Reference analog: GPUHistMakerDevice::UpdateTree,
// src/tree/updater_gpu_hist.cu:588 — the reference's driver is C++
// too; grower.py's Python driver remains for the feature-rich paths:
// categorical splits, column sampling, interaction constraints,
// lossguide growth, external memory.)
//
// Depthwise growth, numeric splits, optional monotone constraints.
// Produces bit-identical trees to the Python GPU driver: same kernels,
// same double-precision host math, compiled with -ffp-contract=off.
//
// gbt_grow_tree packs its arguments, picks one of two modes over a
// shared set of helpers, and runs the shared epilogue:
//  - GrowWholeTree (the main path): ONE host sync per TREE.  Every
//    level's phase chain
//      apply-splits -> partition -> child-hist task generation -> hist
//      build -> sibling subtraction -> split evaluation
//    is enqueued (or replayed as one hipGraph) with every decision made
//    on device; one readback returns the per-level records and the host
//    replays them into the tree arrays.
//  - GrowPerLevel (max_depth 1, trees too deep for the arena, or no
//    device max-abs): ONE host sync per LEVEL.  The same phase chain is
//    enqueued in a single burst per level, then one
//    hipStreamSynchronize reads back the per-node best splits AND the
//    partition counters together.  The build-vs-subtract sibling choice
//    uses the hessian sums known from the parent's evaluation (exact row
//    counts are not yet on the host at enqueue time); histogram
//    subtraction is exact int64, so the choice affects only
//    performance, never the resulting tree.
#include "gbt_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

#define HIP_CHECK(x)                                    \
  do {                                                  \
    hipError_t err__ = (x);                             \
    if (err__ != hipSuccess) return -(int)err__;        \
  } while (0)

// gbt_grow_tree's own failure codes (HIP errors come back as -hipError_t,
// which stays far above these).  The two capacity codes are not errors:
// the caller falls back to the Python driver on them.
constexpr int kErrReplayDiverged = -9991;   // host replay != device chain
constexpr int kErrRootTasksCap = -9996;     // root task list > task buffer
constexpr int kErrArenaTooSmall = -9997;    // wt_ws smaller than WtArena
constexpr int kCapacityTaskGenLds = -9998;  // level wider than kMaxSplitNodes
constexpr int kCapacityHistPool = -9999;    // level wider than the hist pool

bool WtGraphDebug() {
  static int v = [] {
    const char* e = getenv("GBT_WT_GRAPH_DEBUG");
    return e ? atoi(e) : 0;
  }();
  return v != 0;
}

struct PinnedRing {
  static constexpr int kSlots = 6;
  void* host[kSlots] = {};
  void* dev[kSlots] = {};
  size_t cap[kSlots] = {};
  int cur = 0;

  int ensure(int slot, size_t bytes) {
    if (cap[slot] >= bytes) return 0;
    size_t want = 4096;
    while (want < bytes) want <<= 1;
    if (host[slot]) hipHostFree(host[slot]);
    if (dev[slot]) hipFree(dev[slot]);
    HIP_CHECK(hipHostMalloc(&host[slot], want));
    HIP_CHECK(hipMalloc(&dev[slot], want));
    cap[slot] = want;
    return 0;
  }
  int next() {
    int s = cur;
    cur = (cur + 1) % kSlots;
    return s;
  }
};

typedef std::vector<unsigned long long> GraphKey;

struct DriverCtx {
  PinnedRing ring;
  void* readback_host = nullptr;
  size_t readback_cap = 0;

  // hipGraph replay of the single-GPU whole-tree chain: the enqueue
  // sequence is identical every round (no host decisions mid-chain), so
  // after one capture the ~25 launches/tree replay as ONE graph launch.
  // Valid only while every baked address is unchanged — wt_key records
  // them all and any mismatch forces a recapture.  The chain needs no
  // host staging: its per-tree constants are written by its init kernel.
  hipGraphExec_t wt_graph = nullptr;
  GraphKey wt_key;
  // capture-on-second-sight: a key must repeat once before we pay the
  // capture+instantiate cost (fresh per-round contexts — e.g. the gpu
  // approx path rebuilds its ops every iteration — would otherwise
  // capture every round and never replay)
  GraphKey wt_seen_key;
  // capture needs a REAL stream: the caller usually passes torch's
  // default stream (0), and capturing a null-stream alias leaves the
  // legacy stream wedged in capture state.  The chain runs on this
  // dedicated stream, ordered behind the caller stream by gevent.
  hipStream_t gstream = nullptr;
  hipEvent_t gevent = nullptr;

  int ensure_gstream() {
    if (gstream == nullptr)
      HIP_CHECK(hipStreamCreateWithFlags(&gstream, hipStreamNonBlocking));
    if (gevent == nullptr)
      HIP_CHECK(hipEventCreateWithFlags(&gevent, hipEventDisableTiming));
    return 0;
  }

  // Order the graph stream behind the caller stream (staged
  // gradient/root-sum copies enqueued by the wrapper).  HOST-side
  // wait: a hipStreamWaitEvent dependency is not reliably honored
  // by hipGraphLaunch on the target stream (observed: replays read
  // half-staged gradients), and the whole chain is about to run for
  // ~0.5 ms anyway, so the few-us host block is in the noise.
  int wait_for(hipStream_t caller) {
    HIP_CHECK(hipEventRecord(gevent, caller));
    HIP_CHECK(hipEventSynchronize(gevent));
    return 0;
  }

  void drop_graph() {
    if (wt_graph) (void)hipGraphExecDestroy(wt_graph);
    wt_graph = nullptr;
    wt_key.clear();
  }

  // Launch the cached graph on gstream if it was captured for exactly
  // this key.  False = nothing was enqueued (a failed launch also drops
  // the graph).
  bool try_replay(const GraphKey& key) {
    if (wt_graph == nullptr || key != wt_key) return false;
    if (hipGraphLaunch(wt_graph, gstream) == hipSuccess) {
      if (WtGraphDebug()) fprintf(stderr, "[wtgraph] replay\n");
      return true;
    }
    (void)hipGetLastError();
    drop_graph();
    return false;
  }

  // Capture enqueue(gstream) into a graph, instantiate and launch it —
  // unless this is the first sighting of the key, which is only
  // remembered.  *launched says whether the chain now runs on gstream; a
  // capture enqueues nothing for execution, so on every failure path it
  // stays false and the caller enqueues directly.  Nonzero return: the
  // enqueue callable itself failed.
  template <typename Enqueue>
  int capture_and_launch(const GraphKey& key, Enqueue&& enqueue,
                         bool* launched) {
    *launched = false;
    if (key != wt_seen_key) {
      // first sighting of this configuration: run direct, remember it
      wt_seen_key = key;
    } else if (hipStreamBeginCapture(gstream, hipStreamCaptureModeRelaxed) !=
               hipSuccess) {
      (void)hipGetLastError();
    } else {
      int ec = enqueue(gstream);
      hipGraph_t g = nullptr;
      hipError_t ce = hipStreamEndCapture(gstream, &g);
      if (WtGraphDebug())
        fprintf(stderr, "[wtgraph] capture ec=%d end=%d\n", ec, (int)ce);
      if (ec != 0) {
        if (g) (void)hipGraphDestroy(g);
        return ec;
      }
      if (ce == hipSuccess && g != nullptr) {
        drop_graph();
        hipError_t ie = hipGraphInstantiate(&wt_graph, g, nullptr, nullptr, 0);
        hipError_t le = ie == hipSuccess ? hipGraphLaunch(wt_graph, gstream)
                                         : hipErrorUnknown;
        if (WtGraphDebug())
          fprintf(stderr, "[wtgraph] inst=%d launch=%d\n", (int)ie, (int)le);
        if (ie == hipSuccess && le == hipSuccess) {
          wt_key = key;
          *launched = true;
        } else {
          drop_graph();
        }
        (void)hipGraphDestroy(g);
      } else {
        (void)hipGetLastError();
      }
    }
    if (!*launched) {
      // safety: never leave the graph stream wedged mid-capture
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(gstream, &st) == hipSuccess &&
          st != hipStreamCaptureStatusNone) {
        hipGraph_t junk = nullptr;
        (void)hipStreamEndCapture(gstream, &junk);
        if (junk) (void)hipGraphDestroy(junk);
      }
    }
    return 0;
  }

  int ensure_readback(size_t bytes) {
    if (readback_cap >= bytes) return 0;
    size_t want = 4096;
    while (want < bytes) want <<= 1;
    if (readback_host) hipHostFree(readback_host);
    HIP_CHECK(hipHostMalloc(&readback_host, want));
    readback_cap = want;
    return 0;
  }
  ~DriverCtx() {
    for (int i = 0; i < PinnedRing::kSlots; ++i) {
      if (ring.host[i]) hipHostFree(ring.host[i]);
      if (ring.dev[i]) hipFree(ring.dev[i]);
    }
    if (readback_host) hipHostFree(readback_host);
    if (wt_graph) (void)hipGraphExecDestroy(wt_graph);
    if (gstream) (void)hipStreamDestroy(gstream);
    if (gevent) (void)hipEventDestroy(gevent);
  }
};

// hipGraph replay of the whole-tree chain (default on; GBT_WT_GRAPH=0
// disables).  Single-GPU only: the distributed chain interleaves RCCL
// enqueues through a host callback, which a capture cannot contain.
bool WtGraphEnabled() {
  static int v = [] {
    const char* e = getenv("GBT_WT_GRAPH");
    return e ? atoi(e) : 1;
  }();
  return v != 0;
}

// hist wants FEWER, BIGGER tasks than partition: every block pays a
// full LDS zero+flush of the group histogram, so rows/task must
// amortize ~2*group_bins atomics (env GBT_HIST_TASKS to tune)
constexpr long long kHistMinRows = 2048;
long long HistTasksTarget() {
  static long long v = [] {
    const char* e = getenv("GBT_HIST_TASKS");
    long long t = e ? atoll(e) : 256;  // swept: 256 beats 512 by ~4%
                                       // under whole-tree mode
    return t >= 64 && t <= 16384 ? t : 256;
  }();
  return v;
}

// partition task granularity (whole-tree chain): every block makes one
// returning atomic pair on its node's counter line, so at the top
// levels the block count, not the traffic, sets the kernel time.
// Swept 1024 / 2048 / 4096 / 8192: 975 / 1018 / 1023 / 892 rounds/s
// (profiles/r03_bench_kernels_chain.md); 4096 is the largest task of
// the partition kernel's register path.  Env GBT_PART_ROWS to tune; a
// power of two.
long long PartMinRows() {
  static long long v = [] {
    const char* e = getenv("GBT_PART_ROWS");
    long long r = e ? atoll(e) : 4096;
    return r >= 1024 && r <= 65536 && (r & (r - 1)) == 0 ? r : 4096;
  }();
  return v;
}

struct Node {
  int nid;
  int seg_begin, seg_end;
  long long gq, hq;
  int hist_slot;
  double lo, hi;       // monotone weight bounds
  double gain;         // best-split candidate
  int bin, dir, feature;
  long long lgq, lhq;
};

// Leaf weight.  ONE definition for the host replay and ApplyKernel: same
// doubles, same op order, -ffp-contract=off ⇒ the whole-tree replay
// reproduces the device bounds bit-exactly.
__host__ __device__ inline double CalcWeight(double g, double h, double lam,
                                             double alpha, double mds) {
  double t = g;  // L1 threshold
  if (alpha != 0.0) {
    double s = (g > 0.0) ? 1.0 : ((g < 0.0) ? -1.0 : 0.0);
    double m = fabs(g) - alpha;
    if (m < 0.0) m = 0.0;
    t = s * m;
  }
  double w = -t / (h + lam);
  if (mds > 0.0) w = fmin(fmax(w, -mds), mds);
  return w;
}

// fixed-point scale of one gradient component from its max-abs
__host__ __device__ inline double ScaleFromMaxAbs(float maxabs) {
  return maxabs > 0.f ? 1073741824.0 / (double)maxabs : 1.0;
}

// Expansion rule, host and device.  The two MUST agree, or the host
// replay of a whole-tree chain diverges from what the device expanded:
// expand iff gain > 0 (validity) AND gain >= gamma (reference
// driver.h:37 prunes loss_chg < min_split_loss, boundary included).  The
// host sees a record through DecodeBest, which has already folded
// "bin < 0 or non-finite" into gain = -inf; the device reads it raw.
bool ShouldExpand(double gain, double gamma) {
  return gain > 0.0 && gain >= gamma && std::isfinite(gain);
}
__device__ inline bool DevShouldExpand(long long bin, double gain,
                                       double gamma) {
  return bin >= 0 && isfinite(gain) && gain > 0.0 && gain >= gamma;
}

// one best-split record {gain bits, bin, dir, left gq, left hq, feature}
void DecodeBest(const int64_t rec[6], Node* nd) {
  double gain;
  memcpy(&gain, &rec[0], sizeof(double));
  nd->bin = (int)rec[1];
  nd->dir = (int)rec[2];
  nd->lgq = rec[3];
  nd->lhq = rec[4];
  nd->feature = (int)rec[5];
  nd->gain = (nd->bin >= 0 && std::isfinite(gain)) ? gain : -INFINITY;
}

void ChunkTasks(const std::vector<Node*>& nodes, std::vector<BlockTask>* out,
                long long min_rows = 1024, long long target_tasks = 2048) {
  out->clear();
  long long total = 0;
  for (auto* n : nodes) total += n->seg_end - n->seg_begin;
  long long rows_per_task =
      std::max<long long>(min_rows, (total + target_tasks - 1) / target_tasks);
  for (size_t i = 0; i < nodes.size(); ++i) {
    int b = nodes[i]->seg_begin;
    while (b < nodes[i]->seg_end) {
      int e = (int)std::min<long long>(b + rows_per_task, nodes[i]->seg_end);
      out->push_back(BlockTask{(int)i, b, e, 0});
      b = e;
    }
  }
  if (out->empty()) out->push_back(BlockTask{0, 0, 0, 0});
}

__global__ void ZeroI64Kernel(int64_t* p, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = 0;
}

__global__ void IotaKernel(int32_t* r, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x) r[i] = (int)i;
}

// root hist tasks of a [0, n_rows) segment: same layout as ChunkTasks
// over the single root node
long long RootRowsPerTask(long long n_rows, long long min_rows,
                          long long target_tasks) {
  return std::max<long long>(min_rows,
                             (n_rows + target_tasks - 1) / target_tasks);
}
int RootTaskCount(long long n_rows, long long rpt) {
  return (int)std::max<long long>(1, (n_rows + rpt - 1) / rpt);
}

// Whole-tree chain head: row-id iota + root-histogram zero + every
// per-tree constant the chain used to stage from the host (they depend
// only on the configuration): kn=1, kp=0, the root segment, the root
// hist task list.  Block 0 also copies the root sums and gradient
// max-abs into the readback span so ONE D2H copy returns everything.
__global__ void WtInitKernel(int32_t* r, long long n, int64_t* zero,
                             long long zero_n, int32_t* kn, int32_t* kp,
                             int32_t* seg, BlockTask* root_tasks,
                             int n_root_tasks, long long rpt,
                             const int64_t* __restrict__ root_sums,
                             const float* __restrict__ maxabs,
                             int64_t* rs_out /* [2] sums + 2 floats */) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n; i += stride) r[i] = (int)i;
  for (long long i = i0; i < zero_n; i += stride) zero[i] = 0;
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) {
    kn[0] = 1;
    kp[0] = 0;
    seg[0] = 0;
    seg[1] = (int)n;
    rs_out[0] = root_sums[0];
    rs_out[1] = root_sums[1];
    float* ma = (float*)(rs_out + 2);
    ma[0] = maxabs[0];
    ma[1] = maxabs[1];
  }
  for (int t = threadIdx.x; t < n_root_tasks; t += blockDim.x) {
    const long long b = (long long)t * rpt;
    root_tasks[t] =
        BlockTask{0, (int)b, (int)std::min<long long>(b + rpt, n), 0};
  }
}

__global__ void SubtractHistKernel(const int64_t* __restrict__ parents,
                                   const int64_t* __restrict__ built,
                                   int64_t* __restrict__ out,
                                   const int32_t* __restrict__ parent_slot,
                                   int n_bins2, int k,
                                   int64_t* __restrict__ ps,
                                   const int64_t* __restrict__ parent_ps,
                                   const int32_t* __restrict__ kp_dev) {
  if (kp_dev != nullptr) {
    k = *kp_dev;
    out += (long long)k * n_bins2;  // subtracted slots follow the built
  }
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // piggybacked: subtracted-sibling sums = parent - built (slots k..2k-1)
  if (ps != nullptr && idx < k) {
    ps[2 * (k + idx)] = parent_ps[2 * idx] - ps[2 * idx];
    ps[2 * (k + idx) + 1] = parent_ps[2 * idx + 1] - ps[2 * idx + 1];
  }
  const long long total = (long long)k * n_bins2;
  for (long long i = idx; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i / n_bins2);
    const int col = (int)(i % n_bins2);
    out[(long long)row * n_bins2 + col] =
        parents[(long long)parent_slot[row] * n_bins2 + col] -
        built[(long long)row * n_bins2 + col];
  }
}

// widest level the single-block task kernels serve (their LDS arrays)
constexpr int kMaxSplitNodes = 2048;

// Split k row segments [s_begin[j], s_end[j]) (LDS arrays the caller has
// written; this syncs before reading them) into BlockTasks of one common
// power-of-two size and pad the list with empty tasks up to max_tasks
// (the hist/partition kernels early-return on them).  Called by every
// thread of a single-block kernel; k <= kMaxSplitNodes, k == 0 pads all.
__device__ inline void SplitSegmentsIntoTasks(
    const int* s_begin, const int* s_end, int k, long long min_rows,
    long long target_tasks, int max_tasks, BlockTask* __restrict__ out_tasks) {
  __shared__ int s_pref[kMaxSplitNodes];  // first task of each segment
  __shared__ long long s_rpt;
  __shared__ int s_total_tasks;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int j = 0; j < k; ++j) total += s_end[j] - s_begin[j];
    // round rows/task UP to a power of two: all the per-node
    // ceil-divides below become shifts (serial thread-0 64-bit
    // divisions measured ~2x the whole kernel's budget), and the
    // task layout has no effect on results (atomics are
    // order-independent)
    long long rpt0 =
        std::max(min_rows, (total + target_tasks - 1) / target_tasks);
    int shift = 0;
    while ((1LL << shift) < rpt0) ++shift;
    for (;;) {  // defensive: never overflow the task buffer
      long long need = 0;
      for (int j = 0; j < k; ++j) {
        const long long sz = s_end[j] - s_begin[j];
        need += (sz + (1LL << shift) - 1) >> shift;
      }
      if (need <= max_tasks) break;
      ++shift;
    }
    const long long rpt = 1LL << shift;
    int pref = 0;
    for (int j = 0; j < k; ++j) {
      s_pref[j] = pref;
      const long long sz = s_end[j] - s_begin[j];
      pref += (int)((sz + rpt - 1) >> shift);
    }
    s_rpt = rpt;
    s_total_tasks = pref;
  }
  __syncthreads();
  const long long rpt = s_rpt;
  const int total_tasks = s_total_tasks;
  for (int t = threadIdx.x; t < max_tasks; t += blockDim.x) {
    if (t >= total_tasks) {
      out_tasks[t] = BlockTask{0, 0, 0, 0};
      continue;
    }
    // binary search: largest j with prefix[j] <= t
    int lo = 0, hi = k - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_pref[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int j = lo;
    const long long idx = t - s_pref[j];
    const int b = s_begin[j] + (int)(idx * rpt);
    const int e = (int)std::min<long long>((long long)b + rpt,
                                           (long long)s_end[j]);
    out_tasks[t] = BlockTask{j, b, e, 0};
  }
}

// Generate the child-hist BlockTask array on device: the child
// segments come from the partition counters (still in flight on the
// stream when the host enqueues this), so the host never has to wait
// for the partition before launching the hist build.
//   desc[j] = {parent_begin, parent_end, counter_slot, is_left}
// Child j's segment: left  -> [parent_begin, counters[2*slot])
//                    right -> [counters[2*slot], parent_end)
// The task array is padded with empty tasks up to max_tasks.
__global__ void HistTaskGenKernel(const int32_t* __restrict__ counters,
                                  const int32_t* __restrict__ desc, int k,
                                  long long min_rows, long long target_tasks,
                                  int max_tasks,
                                  BlockTask* __restrict__ out_tasks,
                                  int64_t* __restrict__ ps /* [2k][2] to
                                      zero, or null */,
                                  const int32_t* __restrict__ kp_dev,
                                  int32_t* __restrict__ seg_out,
                                  /* null, or [2k][2] child segments in
                                     SLOT order: built j, subtracted
                                     k+j (whole-tree mode) */
                                  int zero_n, /* distributed whole-tree:
                                     zero ps up to this host-known
                                     worst-case bound so the padded
                                     fixed-count allreduce sums zeros,
                                     never stale ping-pong garbage */
                                  uint8_t* __restrict__ mode_out
                                  /* null, or [k]: resolved built-is-left
                                     flag per pair — the EXPLICIT record
                                     of which sibling was built (segment
                                     adjacency is ambiguous for nodes
                                     whose local shard is empty) */) {
  if (kp_dev != nullptr) k = *kp_dev;
  if (ps != nullptr) {
    const int zn = max(4 * k, zero_n);
    for (int i = threadIdx.x; i < zn; i += blockDim.x) ps[i] = 0;
  }
  // parallel load phase: thread-0 doing k dependent global loads costs
  // more than the whole rest of the kernel; gather child segments into
  // LDS cooperatively first (k is capped by the driver's level guard)
  __shared__ int s_begin[kMaxSplitNodes], s_end[kMaxSplitNodes];
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const int pb = desc[4 * j], pe = desc[4 * j + 1];
    const int split = counters[2 * desc[4 * j + 2]];
    // mode: 1 = build left, 0 = build right, 2 = build the smaller
    // child (single-GPU only: local row counts are rank-dependent)
    int mode = desc[4 * j + 3];
    if (mode == 2) mode = (split - pb) <= (pe - split) ? 1 : 0;
    s_begin[j] = mode ? pb : split;
    s_end[j] = mode ? split : pe;
    if (mode_out != nullptr) mode_out[j] = (uint8_t)mode;
    if (seg_out != nullptr) {
      seg_out[2 * j] = s_begin[j];
      seg_out[2 * j + 1] = s_end[j];
      // the subtracted sibling is the complement range
      seg_out[2 * (k + j)] = mode ? split : pb;
      seg_out[2 * (k + j) + 1] = mode ? pe : split;
    }
  }
  SplitSegmentsIntoTasks(s_begin, s_end, k, min_rows, target_tasks, max_tasks,
                         out_tasks);
}

// Whole-tree mode: apply one level's split decisions entirely on
// device.  Reads the level's best-split records and segments, compacts
// the expanding nodes IN PAIR ORDER (left0, right0, left1, ...) so the
// host replay and the python driver number children identically, and
// emits everything the next phase chain needs: partition args + padded
// task list, counters, task-gen descriptors, and the gathered parent
// pair-sums for the sibling-subtraction derivation.
__global__ __launch_bounds__(256) void ApplyKernel(
    const int64_t* __restrict__ best,    // [kn][6] this level's nodes
    const int32_t* __restrict__ segs,    // [kn][2] slot order
    const int32_t* __restrict__ kn_dev,  // node count of this level
    const int32_t* __restrict__ kp_prev_dev,  // pair count (0 at root)
    const int64_t* __restrict__ ps_prev,      // [kn][2] node pair sums
    double gamma_, const int32_t* __restrict__ cut_ptrs,
    long long min_rows, long long target_tasks, int max_ptasks,
    int32_t* __restrict__ kn_out, int32_t* __restrict__ kp_out,
    int32_t* __restrict__ feat, int32_t* __restrict__ sbin,
    uint8_t* __restrict__ dl, int32_t* __restrict__ cnt,
    BlockTask* __restrict__ out_tasks, int32_t* __restrict__ desc,
    int64_t* __restrict__ parent_ps, int32_t* __restrict__ parent_slot,
    // distributed / monotone extensions (all null / 0 otherwise):
    int choice_global,  // 1: build the smaller-GLOBAL-hessian child so
                        // every rank builds (and allreduces) the SAME
                        // sibling slot; 0: HistTaskGenKernel picks the
                        // smaller LOCAL-row child (single-GPU only)
    const float* __restrict__ maxabs,     // [2] scale derivation (mono)
    const int8_t* __restrict__ monotone,  // [F] or null
    double lam, double alpha, double mds,
    const double* __restrict__ bounds_prev,  // [kn][2] slot order | null
    double* __restrict__ bounds_out,         // [2kb][2] slot order | null
    const uint8_t* __restrict__ mode_prev) { // [kp_prev] built-is-left
                                             // flags of the PREVIOUS
                                             // level's pairs, or null
                                             // (root / legacy adjacency)
  __shared__ int s_order[kMaxSplitNodes];   // slots in pair order
  __shared__ uint8_t s_flag[kMaxSplitNodes];
  __shared__ int s_exp[kMaxSplitNodes];     // expanding slots (pair order)
  __shared__ int s_b[kMaxSplitNodes], s_e[kMaxSplitNodes];
  __shared__ int s_kb;
  const int kn = *kn_dev;
  const int kp_prev = *kp_prev_dev;
  // pair-order slot sequence: pair p = slots (p, kp_prev + p); left is
  // the one whose end == the other's begin
  if (kp_prev == 0) {
    if (threadIdx.x == 0) s_order[0] = 0;  // root
  } else {
    for (int p = threadIdx.x; p < kp_prev; p += blockDim.x) {
      const int a = p, b = kp_prev + p;
      // which slot is the LEFT child: from the explicit built-is-left
      // record when available (segment adjacency is ambiguous when this
      // rank's local shard of the pair is empty — distributed mode)
      const bool a_left = mode_prev != nullptr
                              ? (mode_prev[p] != 0)
                              : (segs[2 * a + 1] == segs[2 * b]);
      s_order[2 * p] = a_left ? a : b;
      s_order[2 * p + 1] = a_left ? b : a;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kn; i += blockDim.x) {
    const int slot = s_order[i];
    s_flag[i] = DevShouldExpand(best[6 * slot + 1],
                                __longlong_as_double(best[6 * slot]), gamma_)
                    ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int kb = 0;
    for (int i = 0; i < kn; ++i) {
      if (s_flag[i]) s_exp[kb++] = s_order[i];
    }
    s_kb = kb;
    *kp_out = kb;
    *kn_out = 2 * kb;
  }
  __syncthreads();
  const int kb = s_kb;
  for (int j = threadIdx.x; j < kb; j += blockDim.x) {
    const int e = s_exp[j];
    const int f = (int)best[6 * e + 5];
    const int sb = segs[2 * e], se = segs[2 * e + 1];
    feat[j] = f;
    sbin[j] = (int)best[6 * e + 1] - cut_ptrs[f];
    dl[j] = (uint8_t)best[6 * e + 2];
    cnt[2 * j] = sb;
    cnt[2 * j + 1] = se;
    desc[4 * j] = sb;
    desc[4 * j + 1] = se;
    desc[4 * j + 2] = j;
    const long long pgq = ps_prev[2 * e], phq = ps_prev[2 * e + 1];
    const long long lgq = best[6 * e + 3], lhq = best[6 * e + 4];
    int mode = 2;  // device picks the smaller LOCAL child
    if (choice_global) {
      // rank-identical: global hessians come from the (allreduced)
      // histogram's best record, so every rank builds the same slot
      mode = (lhq <= phq - lhq) ? 1 : 0;
    }
    desc[4 * j + 3] = mode;
    parent_ps[2 * j] = pgq;
    parent_ps[2 * j + 1] = phq;
    parent_slot[j] = e;
    s_b[j] = sb;
    s_e[j] = se;
    if (bounds_out != nullptr) {
      // monotone bound propagation (same math as ApplySplitHost): child
      // bounds in SLOT order — built j, subtracted kb+j
      double lo = bounds_prev ? bounds_prev[2 * e] : -INFINITY;
      double hi = bounds_prev ? bounds_prev[2 * e + 1] : INFINITY;
      double llo = lo, lhi = hi, rlo = lo, rhi = hi;
      const int c = monotone ? (int)monotone[f] : 0;
      if (c != 0) {
        const double ig = 1.0 / ScaleFromMaxAbs(maxabs[0]);
        const double ih = 1.0 / ScaleFromMaxAbs(maxabs[1]);
        double wl = CalcWeight(lgq * ig, lhq * ih, lam, alpha, mds);
        double wr = CalcWeight((pgq - lgq) * ig, (phq - lhq) * ih, lam,
                               alpha, mds);
        wl = fmin(fmax(wl, lo), hi);
        wr = fmin(fmax(wr, lo), hi);
        const double mid = (wl + wr) / 2.0;
        if (c > 0) {
          lhi = fmin(hi, mid);
          rlo = fmax(lo, mid);
        } else {
          llo = fmax(lo, mid);
          rhi = fmin(hi, mid);
        }
      }
      const bool built_left = (mode == 1);
      bounds_out[2 * j] = built_left ? llo : rlo;
      bounds_out[2 * j + 1] = built_left ? lhi : rhi;
      bounds_out[2 * (kb + j)] = built_left ? rlo : llo;
      bounds_out[2 * (kb + j) + 1] = built_left ? rhi : lhi;
    }
  }
  // partition tasks over the expand segments, padded to max_ptasks
  SplitSegmentsIntoTasks(s_b, s_e, kb, min_rows, target_tasks, max_ptasks,
                         out_tasks);
}

struct LeafSeg {
  int nid, begin, end;
  int parity;  // which ping-pong ridx buffer holds these rows
};

typedef void (*AllreduceFn)(long long* dev_ptr, long long n_elems);

// gbt_grow_tree's inputs, in its parameter order (documented there)
struct GrowArgs {
  DriverCtx* ctx;
  const uint8_t* gidx8;
  const uint16_t* gidx16;
  int n_features;
  const uint8_t* gidx8_col;
  const uint16_t* gidx16_col;
  long long n_rows;
  const int32_t* qgpair;
  const int32_t* cut_ptrs_dev;
  const float* cut_values_host;
  const int32_t* cut_ptrs_host;
  const int32_t* n_bins_feat_dev;
  const int32_t* feat_group_start_dev;
  const int32_t* bin_group_start_dev;
  int n_groups, max_group_bins, use_shared, n_bins;
  int32_t* ridx;
  int32_t* ridx_out;
  int64_t* hist_pool_a;
  int64_t* hist_pool_b;
  double* eval_gain;
  int32_t* eval_bin;
  uint8_t* eval_dir;
  int64_t* eval_lsum;
  int64_t* eval_best;
  int32_t* pos_out;
  int max_nodes_level;
  BlockTask* hist_tasks_dev;
  int hist_tasks_cap;
  void* wt_ws;
  long long wt_ws_bytes;
  int wt_max_ptasks;
  const int64_t* root_sums_dev;
  const float* maxabs_dev;
  double* out_scales;
  double g_scale, h_scale;  // host scales; superseded by maxabs_dev's
  double reg_lambda, reg_alpha, max_delta_step, min_child_weight, gamma, eta;
  int max_depth;
  const int8_t* monotone_dev;
  const int8_t* monotone_host;
  const uint8_t* fmask_dev;
  AllreduceFn allreduce;
  hipStream_t stream;

  bool has_mono() const { return monotone_host != nullptr; }
  long long hist_row() const { return (long long)n_bins * 2; }
};

// host tree outputs (caller-sized to 2^(max_depth+1))
struct TreeOut {
  int32_t* left;
  int32_t* right;
  int32_t* parent;
  int32_t* split_index;
  float* split_cond;
  uint8_t* default_left;
  double* loss_chg;
  float* sum_hess;
  float* base_weight;
  int n_tree_nodes;
};

struct Scales {
  double g, h, inv_g, inv_h;
  Scales(double g_scale, double h_scale)
      : g(g_scale), h(h_scale), inv_g(1.0 / g_scale), inv_h(1.0 / h_scale) {}
};

// Root bookkeeping once its sums, best record and (when the scales are
// derived from the gradients' max-abs) max-abs pair are on the host.
void FinishRoot(const GrowArgs& a, const int64_t* root_sums,
                const float* maxabs /* or null */, const int64_t* best,
                Scales* sc, Node* root, TreeOut* out) {
  if (maxabs != nullptr) {
    *sc = Scales(ScaleFromMaxAbs(maxabs[0]), ScaleFromMaxAbs(maxabs[1]));
    if (a.out_scales != nullptr) {
      a.out_scales[0] = sc->g;
      a.out_scales[1] = sc->h;
    }
  }
  root->gq = root_sums[0];
  root->hq = root_sums[1];
  out->base_weight[0] =
      (float)CalcWeight(root->gq * sc->inv_g, root->hq * sc->inv_h,
                        a.reg_lambda, a.reg_alpha, a.max_delta_step);
  out->sum_hess[0] = (float)(root->hq * sc->inv_h);
  DecodeBest(best, root);
}

// Apply one split on the host: number the two children, write the tree
// arrays, clamp the child weights to the node's bounds and propagate
// the monotone bounds — bit-identical to ApplyKernel's fp64 math.  The
// children's sums and bounds are known from the parent's evaluation;
// their segments and best splits arrive later.
void ApplySplitHost(const GrowArgs& a, const Scales& sc, const Node& nd,
                    TreeOut* out, Node* ln, Node* rn) {
  const int l = out->n_tree_nodes, r = out->n_tree_nodes + 1;
  out->n_tree_nodes += 2;
  out->left[nd.nid] = l;
  out->right[nd.nid] = r;
  out->left[l] = out->right[l] = -1;
  out->left[r] = out->right[r] = -1;
  out->parent[l] = nd.nid;
  out->parent[r] = nd.nid;
  out->split_index[nd.nid] = nd.feature;
  out->split_cond[nd.nid] = a.cut_values_host[nd.bin];
  out->default_left[nd.nid] = (uint8_t)nd.dir;
  out->loss_chg[nd.nid] = nd.gain;
  const long long rgq = nd.gq - nd.lgq, rhq = nd.hq - nd.lhq;
  double wl = CalcWeight(nd.lgq * sc.inv_g, nd.lhq * sc.inv_h, a.reg_lambda,
                         a.reg_alpha, a.max_delta_step);
  double wr = CalcWeight(rgq * sc.inv_g, rhq * sc.inv_h, a.reg_lambda,
                         a.reg_alpha, a.max_delta_step);
  wl = std::fmin(std::fmax(wl, nd.lo), nd.hi);
  wr = std::fmin(std::fmax(wr, nd.lo), nd.hi);
  out->sum_hess[nd.nid] = (float)((nd.lhq + rhq) * sc.inv_h);
  out->base_weight[l] = (float)wl;
  out->base_weight[r] = (float)wr;
  out->sum_hess[l] = (float)(nd.lhq * sc.inv_h);
  out->sum_hess[r] = (float)(rhq * sc.inv_h);
  *ln = Node{};
  *rn = Node{};
  ln->nid = l;
  rn->nid = r;
  ln->gq = nd.lgq;
  ln->hq = nd.lhq;
  rn->gq = rgq;
  rn->hq = rhq;
  ln->seg_begin = ln->seg_end = -1;  // not yet known
  rn->seg_begin = rn->seg_end = -1;
  ln->lo = rn->lo = nd.lo;
  ln->hi = rn->hi = nd.hi;
  ln->gain = rn->gain = -INFINITY;
  ln->bin = rn->bin = -1;
  if (a.has_mono() && nd.feature < a.n_features) {
    const int c = a.monotone_host[nd.feature];
    if (c != 0) {
      const double mid = (wl + wr) / 2.0;
      if (c > 0) {
        ln->hi = std::fmin(nd.hi, mid);
        rn->lo = std::fmax(nd.lo, mid);
      } else {
        ln->lo = std::fmax(nd.lo, mid);
        rn->hi = std::fmin(nd.hi, mid);
      }
    }
  }
}

// One level of host decisions: nodes that stop become leaves (their rows
// sit in the ridx buffer of `parity`), the rest are split into
// next_level in pair order (left0, right0, left1, ...).
void ExpandLevel(const GrowArgs& a, const Scales& sc,
                 std::vector<Node>& level_nodes, int parity, TreeOut* out,
                 std::vector<LeafSeg>* leaves, std::vector<Node*>* expand,
                 std::vector<Node>* next_level) {
  expand->clear();
  for (auto& nd : level_nodes) {
    if (ShouldExpand(nd.gain, a.gamma)) {
      expand->push_back(&nd);
    } else {
      leaves->push_back({nd.nid, nd.seg_begin, nd.seg_end, parity});
    }
  }
  next_level->assign(2 * expand->size(), Node{});
  for (size_t i = 0; i < expand->size(); ++i) {
    ApplySplitHost(a, sc, *(*expand)[i], out, &(*next_level)[2 * i],
                   &(*next_level)[2 * i + 1]);
  }
}

// Final level: the children are all leaves — write their positions
// directly (one decide pass over the parents' rows, host-staged args)
// instead of partition + counter sync + a later leaf sweep.
int StageLeafDecide(const GrowArgs& a, const int32_t* cur_ridx,
                    const std::vector<Node*>& expand,
                    const std::vector<Node>& next_level) {
  const int k = (int)expand.size();
  std::vector<BlockTask> tasks;
  ChunkTasks(expand, &tasks);
  PinnedRing& ring = a.ctx->ring;
  const int slot = ring.next();
  size_t off_feat = (tasks.size() * sizeof(BlockTask) + 7) & ~7ULL;
  size_t off_sbin = (off_feat + (size_t)k * 4 + 7) & ~7ULL;
  size_t off_dl = (off_sbin + (size_t)k * 4 + 7) & ~7ULL;
  size_t off_kids = (off_dl + (size_t)k + 7) & ~7ULL;
  size_t bytes = off_kids + (size_t)k * 8;
  if (int e = ring.ensure(slot, bytes)) return e;
  char* h = (char*)ring.host[slot];
  memcpy(h, tasks.data(), tasks.size() * sizeof(BlockTask));
  int32_t* feat = (int32_t*)(h + off_feat);
  int32_t* sbin = (int32_t*)(h + off_sbin);
  uint8_t* dl = (uint8_t*)(h + off_dl);
  int32_t* kids = (int32_t*)(h + off_kids);
  for (int j = 0; j < k; ++j) {
    const Node* nd = expand[j];
    feat[j] = nd->feature;
    sbin[j] = nd->bin - a.cut_ptrs_host[nd->feature];
    dl[j] = (uint8_t)nd->dir;
    kids[2 * j] = next_level[2 * j].nid;
    kids[2 * j + 1] = next_level[2 * j + 1].nid;
  }
  HIP_CHECK(hipMemcpyAsync(ring.dev[slot], h, bytes, hipMemcpyHostToDevice,
                           a.stream));
  char* d = (char*)ring.dev[slot];
  gbt_leaf_decide(a.gidx8, a.gidx16, a.n_features, a.gidx8_col, a.gidx16_col,
                  a.n_rows, cur_ridx, (const BlockTask*)d, (int)tasks.size(),
                  (const int32_t*)(d + off_feat),
                  (const int32_t*)(d + off_sbin),
                  (const uint8_t*)(d + off_dl),
                  (const int32_t*)(d + off_kids), a.n_bins_feat_dev,
                  a.pos_out, a.stream);
  return 0;
}

// ================= WHOLE-TREE MODE =================
// Every level's phase chain — apply-splits, partition, task generation,
// hist, subtraction, evaluation — is enqueued with NO host sync (the
// expansion decision and all task lists are computed on device); ONE
// readback at the end returns the per-level best-split and segment
// records, and the host replays them to build the tree arrays
// (bit-identical: the replay applies the same comparisons to the same
// doubles).
// Distributed (allreduce != null): same single-enqueue chain — the
// per-level hist/pair-sum allreduces are enqueued with a host-known
// WORST-CASE padded count (zero slots reduce to zeros), and the
// sibling build/subtract choice comes from GLOBAL hessians so every
// rank reduces the same slot layout.  Monotone: fp64 bound
// propagation runs inside ApplyKernel (scales derived on device).
// Single-GPU: the fixed launch sequence is captured into a hipGraph
// once and replayed (one graph launch instead of ~25 enqueues/tree).

// Layout of the whole-tree arena (byte offsets into wt_ws).  This is the
// only place that knows it: the caller sizes wt_ws by
// gbt_wt_arena_bytes.
struct WtArena {
  int pool;  // node slots per level record
  // readback span: everything the host replay needs sits contiguously
  // at the head of the arena, so ONE D2H copy of r_total bytes returns it
  size_t o_best, o_seg, o_kp, o_mode, o_rs, r_total;
  // device-only chain arguments
  size_t o_kn, o_desc, o_feat, o_sbin, o_dl, o_cnt, o_ptasks, o_pps, o_pslot;
  size_t o_ps[2], o_bnd[2];
  size_t total;

  // level L's children live in record slots [rec(L), rec(L) + pool);
  // the root is slot 0
  size_t rec(int L) const { return 1 + (size_t)L * pool; }
};

WtArena MakeWtArena(int max_depth, int pool, int wt_max_ptasks,
                    bool has_mono) {
  WtArena ar{};
  ar.pool = pool;
  const size_t rec_slots = ar.rec(max_depth);
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    size_t o = off;
    off = (off + bytes + 255) & ~255ULL;
    return o;
  };
  ar.o_best = carve(rec_slots * 6 * 8);
  ar.o_seg = carve(rec_slots * 2 * 4);
  ar.o_kp = carve((size_t)(max_depth + 2) * 4);
  ar.o_mode = carve((size_t)max_depth * pool);  // [max_depth][pool]
  ar.o_rs = carve(24);  // root sums [2] i64 + max-abs [2] f32
  ar.r_total = ar.o_rs + 24;
  ar.o_kn = carve((size_t)(max_depth + 2) * 4);
  ar.o_desc = carve((size_t)pool * 16);
  ar.o_feat = carve((size_t)pool * 4);
  ar.o_sbin = carve((size_t)pool * 4);
  ar.o_dl = carve((size_t)pool);
  ar.o_cnt = carve((size_t)pool * 8);
  ar.o_ptasks = carve((size_t)wt_max_ptasks * sizeof(BlockTask));
  ar.o_pps = carve((size_t)pool * 16);
  ar.o_pslot = carve((size_t)pool * 4);
  ar.o_ps[0] = carve((size_t)pool * 16);
  ar.o_ps[1] = carve((size_t)pool * 16);
  ar.o_bnd[0] = has_mono ? carve((size_t)pool * 16) : 0;
  ar.o_bnd[1] = has_mono ? carve((size_t)pool * 16) : 0;
  ar.total = off;
  return ar;
}

// what the whole-tree chain bakes at enqueue time besides GrowArgs
struct WtChain {
  WtArena ar;
  char* w;  // arena base
  int n_root_tasks;
  long long root_rpt;
  int wt_max_htasks;
  int n_ptasks;  // partition launch grid: sum over nodes of
                 // ceil(rows / rows-per-task)
  template <typename T>
  T* at(size_t off) const { return (T*)(w + off); }
};

// ---- the chain: EVERY launch for the whole tree, no host sync.
// Ping-pong pointers are locals so a graph REPLAY (which skips this
// code entirely) leaves the caller's state identical.  No host<->device
// copy is part of it (graph-embedded memcpy/memset nodes showed
// unreliable replay ordering on ROCm): constants are written and
// buffers zeroed by kernels.
int EnqueueChain(const GrowArgs& a, const WtChain& c, hipStream_t cs) {
  const WtArena& ar = c.ar;
  const bool has_mono = a.has_mono();
  const int choice_global = (a.allreduce != nullptr || has_mono) ? 1 : 0;
  const long long hist_row = a.hist_row();
  const int pool = ar.pool;
  int64_t* best_rec = c.at<int64_t>(ar.o_best);
  int32_t* seg_rec = c.at<int32_t>(ar.o_seg);
  int32_t* kn_arr = c.at<int32_t>(ar.o_kn);
  int32_t* kp_arr = c.at<int32_t>(ar.o_kp);
  int32_t* d_desc = c.at<int32_t>(ar.o_desc);
  int32_t* d_feat = c.at<int32_t>(ar.o_feat);
  int32_t* d_sbin = c.at<int32_t>(ar.o_sbin);
  uint8_t* d_dl = c.at<uint8_t>(ar.o_dl);
  int32_t* d_cnt = c.at<int32_t>(ar.o_cnt);
  BlockTask* d_pt = c.at<BlockTask>(ar.o_ptasks);
  int64_t* d_pps = c.at<int64_t>(ar.o_pps);
  int32_t* d_pslot = c.at<int32_t>(ar.o_pslot);
  uint8_t* d_mode = c.at<uint8_t>(ar.o_mode);
  int64_t* ps_bufs[2] = {c.at<int64_t>(ar.o_ps[0]), c.at<int64_t>(ar.o_ps[1])};
  double* bnd_bufs[2] = {has_mono ? c.at<double>(ar.o_bnd[0]) : nullptr,
                         has_mono ? c.at<double>(ar.o_bnd[1]) : nullptr};
  const int8_t* mono = has_mono ? a.monotone_dev : nullptr;
  int32_t* cr = a.ridx;
  int32_t* alt = a.ridx_out;
  int64_t* cp = a.hist_pool_a;
  int64_t* np2 = a.hist_pool_b;
  {
    // root hist tasks: a function of the configuration only, written on
    // device into the hist task buffer (the level-0 task generation
    // overwrites it after the root hist has run)
    int blocks = (int)std::min<long long>((a.n_rows + 255) / 256, 4096);
    hipLaunchKernelGGL(WtInitKernel, dim3(std::max(blocks, 1)), dim3(256), 0,
                       cs, cr, a.n_rows, cp, hist_row, kn_arr, kp_arr,
                       seg_rec, a.hist_tasks_dev, c.n_root_tasks, c.root_rpt,
                       a.root_sums_dev, a.maxabs_dev,
                       c.at<int64_t>(ar.o_rs));
  }
  gbt_hist(a.gidx8, a.gidx16, a.n_features, a.qgpair, cr, a.hist_tasks_dev,
           c.n_root_tasks, cp, a.n_bins, a.feat_group_start_dev,
           a.bin_group_start_dev, a.n_groups, a.max_group_bins,
           a.cut_ptrs_dev, a.use_shared, nullptr, cs);
  if (a.allreduce) a.allreduce((long long*)cp, hist_row);
  // root evaluation straight into best_rec[0]
  gbt_evaluate_masked(cp, 1, a.n_bins, a.n_features, a.cut_ptrs_dev,
                      a.root_sums_dev, a.maxabs_dev, 0.0, 0.0, a.reg_lambda,
                      a.reg_alpha, a.max_delta_step, a.min_child_weight, mono,
                      nullptr, 0 /*mask_stride*/, a.fmask_dev, nullptr,
                      a.eval_gain, a.eval_bin, a.eval_dir, a.eval_lsum,
                      nullptr, 0, cs);
  gbt_select_best(a.eval_gain, a.eval_bin, a.eval_dir, a.eval_lsum, 1,
                  a.n_features, best_rec, nullptr, cs);
  const int64_t* ps_prev = a.root_sums_dev;
  for (int L = 0; L + 1 < a.max_depth; ++L) {
    const size_t rec_in = L == 0 ? 0 : ar.rec(L - 1);
    const int64_t* bl = best_rec + rec_in * 6;
    const int32_t* sl = seg_rec + rec_in * 2;
    int64_t* bo = best_rec + ar.rec(L) * 6;
    int32_t* so = seg_rec + ar.rec(L) * 2;
    int64_t* ps_next = ps_bufs[L & 1];
    // level-L capacity: at most 2^L nodes expand, 2^(L+1) children
    const int cap_kids = (int)std::min<long long>(2LL << L, (long long)pool);
    hipLaunchKernelGGL(ApplyKernel, dim3(1), dim3(256), 0, cs, bl, sl,
                       kn_arr + L, kp_arr + L, ps_prev, a.gamma,
                       a.cut_ptrs_dev, PartMinRows(), (long long)2048,
                       c.n_ptasks, kn_arr + L + 1, kp_arr + L + 1, d_feat,
                       d_sbin, d_dl, d_cnt, d_pt, d_desc, d_pps, d_pslot,
                       choice_global, a.maxabs_dev, mono, a.reg_lambda,
                       a.reg_alpha, a.max_delta_step,
                       (L == 0 || !has_mono) ? nullptr
                                             : bnd_bufs[(L - 1) & 1],
                       bnd_bufs[L & 1],
                       L == 0 ? nullptr : d_mode + (size_t)(L - 1) * pool);
    gbt_partition(a.gidx8, a.gidx16, a.n_features, a.gidx8_col, a.gidx16_col,
                  a.n_rows, cr, alt, d_pt, c.n_ptasks, d_feat, d_sbin,
                  d_dl, nullptr, nullptr, a.n_bins_feat_dev, d_cnt, cs);
    std::swap(cr, alt);
    hipLaunchKernelGGL(HistTaskGenKernel, dim3(1), dim3(256), 0, cs, d_cnt,
                       d_desc, 0, kHistMinRows, HistTasksTarget(),
                       c.wt_max_htasks, a.hist_tasks_dev, ps_next,
                       kp_arr + L + 1, so,
                       a.allreduce != nullptr ? 2 * cap_kids : 0,
                       d_mode + (size_t)L * pool);
    {
      // zero via a kernel, not hipMemsetAsync: memset NODES in a
      // captured graph replay out of order on this ROCm
      const long long zn = (long long)cap_kids * hist_row;
      int zb = (int)std::min<long long>((zn + 255) / 256, 4096);
      hipLaunchKernelGGL(ZeroI64Kernel, dim3(zb), dim3(256), 0, cs, np2, zn);
    }
    gbt_hist(a.gidx8, a.gidx16, a.n_features, a.qgpair, cr, a.hist_tasks_dev,
             c.wt_max_htasks, np2, a.n_bins, a.feat_group_start_dev,
             a.bin_group_start_dev, a.n_groups, a.max_group_bins,
             a.cut_ptrs_dev, a.use_shared, ps_next, cs);
    if (a.allreduce) {
      // fixed worst-case counts (host-known, rank-identical): built
      // hist slots 0..cap/2-1 (unused slots are zeros — the zero
      // kernel covers the pool, HistTaskGenKernel zeroed the ps
      // padding)
      // and the built-child pair sums.  Sibling subtraction AFTER
      // the reduce yields global histograms/sums for every child.
      a.allreduce((long long*)np2, (long long)(cap_kids / 2) * hist_row);
      a.allreduce((long long*)ps_next, (long long)cap_kids);
    }
    {
      const long long total = (long long)(cap_kids / 2 + 1) * hist_row;
      int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
      hipLaunchKernelGGL(SubtractHistKernel, dim3(blocks), dim3(256), 0, cs,
                         cp, np2, np2, d_pslot, (int)hist_row, 0, ps_next,
                         d_pps, kp_arr + L + 1);
    }
    gbt_evaluate_masked(np2, cap_kids, a.n_bins, a.n_features, a.cut_ptrs_dev,
                        ps_next, a.maxabs_dev, 0.0, 0.0, a.reg_lambda,
                        a.reg_alpha, a.max_delta_step, a.min_child_weight,
                        mono, bnd_bufs[L & 1], 0 /*mask_stride*/, a.fmask_dev,
                        nullptr, a.eval_gain, a.eval_bin, a.eval_dir,
                        a.eval_lsum, kn_arr + L + 1, 0, cs);
    gbt_select_best(a.eval_gain, a.eval_bin, a.eval_dir, a.eval_lsum,
                    cap_kids, a.n_features, bo, kn_arr + L + 1, cs);
    ps_prev = ps_next;
    std::swap(cp, np2);
  }
  return 0;
}

// The graph key records every address and scalar the chain bakes at
// enqueue time — any change forces a recapture, so replay is exactly
// equivalent.
GraphKey ChainKey(const GrowArgs& a, const WtChain& c) {
  typedef unsigned long long U;
  auto db = [](double d) {
    U u;
    memcpy(&u, &d, 8);
    return u;
  };
  return {(U)a.gidx8, (U)a.gidx16, (U)a.gidx8_col, (U)a.gidx16_col,
          (U)a.qgpair, (U)a.cut_ptrs_dev, (U)a.n_bins_feat_dev,
          (U)a.feat_group_start_dev, (U)a.bin_group_start_dev, (U)a.ridx,
          (U)a.ridx_out, (U)a.hist_pool_a, (U)a.hist_pool_b, (U)a.eval_gain,
          (U)a.eval_bin, (U)a.eval_dir, (U)a.eval_lsum, (U)a.hist_tasks_dev,
          (U)a.wt_ws, (U)a.root_sums_dev, (U)a.maxabs_dev, (U)a.monotone_dev,
          (U)a.fmask_dev, (U)a.ctx->readback_host, (U)a.n_rows,
          (U)a.n_features, (U)a.n_bins, (U)a.use_shared, (U)a.n_groups,
          (U)a.max_group_bins, (U)a.max_depth, (U)a.max_nodes_level,
          (U)a.wt_max_ptasks, (U)a.hist_tasks_cap, (U)c.n_root_tasks,
          (U)c.root_rpt, (U)PartMinRows(), (U)c.n_ptasks, (U)c.wt_max_htasks,
          (U)a.has_mono(), db(a.reg_lambda), db(a.reg_alpha),
          db(a.max_delta_step), db(a.min_child_weight), db(a.gamma)};
}

int GrowWholeTree(const GrowArgs& a, TreeOut* out,
                  std::vector<LeafSeg>* leaves) {
  DriverCtx* ctx = a.ctx;
  WtChain c{};
  c.ar = MakeWtArena(a.max_depth, 2 * a.max_nodes_level, a.wt_max_ptasks,
                     a.has_mono());
  const WtArena& ar = c.ar;
  if ((long long)ar.total > a.wt_ws_bytes) return kErrArenaTooSmall;
  c.w = (char*)a.wt_ws;
  c.root_rpt = RootRowsPerTask(a.n_rows, kHistMinRows, HistTasksTarget());
  c.n_root_tasks = RootTaskCount(a.n_rows, c.root_rpt);
  if (c.n_root_tasks > a.hist_tasks_cap) return kErrRootTasksCap;
  c.wt_max_htasks = (int)std::min<long long>(
      std::min<long long>(a.n_rows / kHistMinRows, HistTasksTarget()) +
          a.max_nodes_level + 1,
      (long long)a.hist_tasks_cap);
  c.n_ptasks = (int)std::min<long long>(
      a.n_rows / PartMinRows() + ar.pool + 2, (long long)a.wt_max_ptasks);
  // pre-size the ONE readback so its (graph-baked) address is final;
  // host offsets equal the arena offsets of the readback span
  if (int e = ctx->ensure_readback(ar.r_total)) return e;
  char* rb = (char*)ctx->readback_host;

  // hipGraph capture/replay (single-GPU only).  Capture and launch run
  // on the ctx-owned stream (never the caller's, which is usually the
  // un-capturable default stream), ordered behind the caller's pending
  // work by a host wait and joined by the host sync.
  bool on_gstream = false;
  if (a.allreduce == nullptr && WtGraphEnabled() &&
      ctx->ensure_gstream() == 0) {
    const GraphKey key = ChainKey(a, c);
    if (int e = ctx->wait_for(a.stream)) return e;
    on_gstream = ctx->try_replay(key);
    if (!on_gstream) {
      auto enqueue = [&](hipStream_t cs) { return EnqueueChain(a, c, cs); };
      if (int e = ctx->capture_and_launch(key, enqueue, &on_gstream)) return e;
    }
  }
  // D2H readback: ONE copy of the arena's readback span, enqueued
  // directly after the kernels (not a graph node); the ONE sync follows
  hipStream_t chain_stream = on_gstream ? ctx->gstream : a.stream;
  if (!on_gstream) {
    if (WtGraphDebug()) fprintf(stderr, "[wtgraph] direct enqueue\n");
    if (int e = EnqueueChain(a, c, a.stream)) return e;
  }
  HIP_CHECK(hipMemcpyAsync(rb, c.w + ar.o_best, ar.r_total,
                           hipMemcpyDeviceToHost, chain_stream));
  if (on_gstream) HIP_CHECK(hipStreamSynchronize(ctx->gstream));
  HIP_CHECK(hipStreamSynchronize(a.stream));

  // ---- host replay of the records ----
  const int64_t* h_best = (const int64_t*)(rb + ar.o_best);
  const int32_t* h_seg = (const int32_t*)(rb + ar.o_seg);
  const int32_t* h_kp = (const int32_t*)(rb + ar.o_kp);
  const uint8_t* h_mode = (const uint8_t*)(rb + ar.o_mode);
  Scales sc(a.g_scale, a.h_scale);
  Node root{};
  root.seg_end = (int)a.n_rows;
  root.lo = -INFINITY;
  root.hi = INFINITY;
  FinishRoot(a, (const int64_t*)(rb + ar.o_rs),
             (const float*)(rb + ar.o_rs + 16), h_best, &sc, &root, out);
  std::vector<Node> level_nodes{root}, next_level;
  std::vector<Node*> expand;
  for (int depth = 0; depth < a.max_depth && !level_nodes.empty(); ++depth) {
    ExpandLevel(a, sc, level_nodes, depth & 1, out, leaves, &expand,
                &next_level);
    if (expand.empty()) break;
    const int kb = (int)expand.size();
    if (depth + 1 >= a.max_depth) {
      // the chain swapped its local ping-pong pointers once per level
      return StageLeafDecide(a, (depth & 1) ? a.ridx_out : a.ridx, expand,
                             next_level);
    }
    if (h_kp[depth + 1] != kb) return kErrReplayDiverged;
    const int64_t* bo = h_best + ar.rec(depth) * 6;
    const int32_t* so = h_seg + ar.rec(depth) * 2;
    const uint8_t* mo = h_mode + (size_t)depth * ar.pool;
    for (int j = 0; j < kb; ++j) {
      // record slots: built child j, subtracted child kb + j
      const bool built_left = mo[j] != 0;
      Node& built = next_level[2 * j + (built_left ? 0 : 1)];
      Node& subtracted = next_level[2 * j + (built_left ? 1 : 0)];
      built.seg_begin = so[2 * j];
      built.seg_end = so[2 * j + 1];
      subtracted.seg_begin = so[2 * (kb + j)];
      subtracted.seg_end = so[2 * (kb + j) + 1];
      DecodeBest(bo + 6 * j, &built);
      DecodeBest(bo + 6 * (kb + j), &subtracted);
    }
    level_nodes.swap(next_level);
  }
  return 0;
}

// ================= PER-LEVEL MODE =================

// Enqueue split evaluation of k nodes against `hists` into eval_best.
// Node sums (and monotone bounds) are staged from `nodes` unless a
// device-resident sum buffer is given (the root's, or device-chosen
// siblings whose sums the GPU computed).
int EvaluateEnqueue(const GrowArgs& a, const Scales& sc, int k,
                    const std::vector<Node*>* nodes, const int64_t* hists,
                    const int64_t* ps_dev, const float* maxabs_eval) {
  const double* bounds_dev = nullptr;
  if (ps_dev == nullptr) {
    const bool has_mono = a.has_mono();
    PinnedRing& ring = a.ctx->ring;
    const int slot = ring.next();
    size_t off_bd = ((size_t)k * 2 * sizeof(int64_t) + 7) & ~7ULL;
    size_t bytes = off_bd + (has_mono ? (size_t)k * 2 * sizeof(double) : 0);
    if (int e = ring.ensure(slot, bytes)) return e;
    char* h = (char*)ring.host[slot];
    int64_t* ps = (int64_t*)h;
    for (int i = 0; i < k; ++i) {
      ps[2 * i] = (*nodes)[i]->gq;
      ps[2 * i + 1] = (*nodes)[i]->hq;
    }
    if (has_mono) {
      double* bd = (double*)(h + off_bd);
      for (int i = 0; i < k; ++i) {
        bd[2 * i] = (*nodes)[i]->lo;
        bd[2 * i + 1] = (*nodes)[i]->hi;
      }
    }
    HIP_CHECK(hipMemcpyAsync(ring.dev[slot], h, bytes, hipMemcpyHostToDevice,
                             a.stream));
    char* d = (char*)ring.dev[slot];
    ps_dev = (const int64_t*)d;
    if (has_mono) bounds_dev = (const double*)(d + off_bd);
  }
  gbt_evaluate_masked(hists, k, a.n_bins, a.n_features, a.cut_ptrs_dev,
                      ps_dev, maxabs_eval, sc.g, sc.h, a.reg_lambda,
                      a.reg_alpha, a.max_delta_step, a.min_child_weight,
                      a.monotone_dev, bounds_dev, 0 /*mask_stride*/,
                      a.fmask_dev, nullptr, a.eval_gain, a.eval_bin,
                      a.eval_dir, a.eval_lsum, nullptr, 0, a.stream);
  gbt_select_best(a.eval_gain, a.eval_bin, a.eval_dir, a.eval_lsum, k,
                  a.n_features, a.eval_best, nullptr, a.stream);
  return 0;
}

// one D2H burst + ONE sync per level: best splits for n_eval nodes +
// partition counters for n_expand nodes
int LevelSync(const GrowArgs& a, int n_eval, int n_expand,
              const int32_t* cnt_dev, const int64_t** best_out,
              const int32_t** cnt_out) {
  size_t off_cnt = ((size_t)n_eval * 6 * sizeof(int64_t) + 63) & ~63ULL;
  size_t bytes = off_cnt + (size_t)n_expand * 2 * sizeof(int32_t);
  if (int e = a.ctx->ensure_readback(bytes)) return e;
  char* h = (char*)a.ctx->readback_host;
  if (n_eval > 0) {
    HIP_CHECK(hipMemcpyAsync(h, a.eval_best,
                             (size_t)n_eval * 6 * sizeof(int64_t),
                             hipMemcpyDeviceToHost, a.stream));
  }
  if (n_expand > 0) {
    HIP_CHECK(hipMemcpyAsync(h + off_cnt, cnt_dev,
                             (size_t)n_expand * 2 * sizeof(int32_t),
                             hipMemcpyDeviceToHost, a.stream));
  }
  HIP_CHECK(hipStreamSynchronize(a.stream));
  *best_out = (const int64_t*)h;
  *cnt_out = (const int32_t*)(h + off_cnt);
  return 0;
}

int GrowPerLevel(const GrowArgs& a, TreeOut* out,
                 std::vector<LeafSeg>* leaves) {
  DriverCtx* ctx = a.ctx;
  PinnedRing& ring = ctx->ring;
  hipStream_t stream = a.stream;
  const long long hist_row = a.hist_row();
  const long long hist_tasks = HistTasksTarget();
  const bool has_mono = a.has_mono();
  Scales sc(a.g_scale, a.h_scale);
  {
    int blocks = (int)std::min<long long>((a.n_rows + 255) / 256, 4096);
    hipLaunchKernelGGL(IotaKernel, dim3(blocks), dim3(256), 0, stream, a.ridx,
                       a.n_rows);
  }
  // ping-pong row-index buffers: the partition scatters cur -> alt and
  // the buffers swap, so no copy-back pass is needed.  Rows of a node
  // that stops expanding stay put in whichever buffer was current at
  // that level (later partitions only write other, disjoint ranges),
  // so each leaf records its buffer parity for the final position pass.
  int32_t* cur_ridx = a.ridx;
  int32_t* alt_ridx = a.ridx_out;
  int64_t* cur_pool = a.hist_pool_a;
  int64_t* next_pool = a.hist_pool_b;

  Node root{};
  root.seg_end = (int)a.n_rows;
  root.lo = -INFINITY;
  root.hi = INFINITY;
  {
    // ---- root histogram: tasks host-generated (root segment is known)
    std::vector<Node*> nodes{&root};
    std::vector<BlockTask> tasks;
    ChunkTasks(nodes, &tasks, kHistMinRows, hist_tasks);
    const int slot = ring.next();
    size_t bytes = tasks.size() * sizeof(BlockTask);
    if (int e = ring.ensure(slot, bytes)) return e;
    memcpy(ring.host[slot], tasks.data(), bytes);
    HIP_CHECK(hipMemcpyAsync(ring.dev[slot], ring.host[slot], bytes,
                             hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(a.hist_pool_a, 0, hist_row * sizeof(int64_t),
                             stream));
    gbt_hist(a.gidx8, a.gidx16, a.n_features, a.qgpair, a.ridx,
             (const BlockTask*)ring.dev[slot], (int)tasks.size(),
             a.hist_pool_a, a.n_bins, a.feat_group_start_dev,
             a.bin_group_start_dev, a.n_groups, a.max_group_bins,
             a.cut_ptrs_dev, a.use_shared, nullptr, stream);
    if (a.allreduce) a.allreduce((long long*)a.hist_pool_a, hist_row);
  }
  {
    // ---- root evaluation (root-only sync; root sums + max-abs ride
    // along, so neither needs its own host round-trip) ----
    if (int e = EvaluateEnqueue(a, sc, 1, nullptr, a.hist_pool_a,
                                a.root_sums_dev, a.maxabs_dev))
      return e;
    const int rslot = ring.next();
    if (int e = ring.ensure(rslot, 4 * sizeof(int64_t))) return e;
    char* rh = (char*)ring.host[rslot];
    HIP_CHECK(hipMemcpyAsync(rh, a.root_sums_dev, 2 * sizeof(int64_t),
                             hipMemcpyDeviceToHost, stream));
    if (a.maxabs_dev != nullptr) {
      HIP_CHECK(hipMemcpyAsync(rh + 2 * sizeof(int64_t), a.maxabs_dev,
                               2 * sizeof(float), hipMemcpyDeviceToHost,
                               stream));
    }
    const int64_t* best;
    const int32_t* cnt;
    if (int e = LevelSync(a, 1, 0, nullptr, &best, &cnt)) return e;
    FinishRoot(a, (const int64_t*)rh,
               a.maxabs_dev != nullptr
                   ? (const float*)(rh + 2 * sizeof(int64_t))
                   : nullptr,
               best, &sc, &root, out);
  }

  std::vector<Node> level_nodes{root}, next_level;
  std::vector<Node*> expand;
  for (int depth = 0; depth < a.max_depth && !level_nodes.empty(); ++depth) {
    // apply splits on host (child sums/bounds are known from the
    // parents' evaluation; child SEGMENTS arrive at the level sync)
    ExpandLevel(a, sc, level_nodes, (cur_ridx == a.ridx) ? 0 : 1, out, leaves,
                &expand, &next_level);
    if (expand.empty()) {
      level_nodes.clear();
      break;
    }
    if (depth + 1 >= a.max_depth) {
      if (int e = StageLeafDecide(a, cur_ridx, expand, next_level)) return e;
      level_nodes.clear();
      break;
    }
    const int kb = (int)expand.size();
    // capacity guards bound the HIST pool slots and the task-gen
    // LDS arrays (the final level above only runs the leaf decide, so
    // up to 2*max_nodes_level nodes may expand there without either)
    if (2 * kb > 2 * a.max_nodes_level) return kCapacityHistPool;
    if (kb > kMaxSplitNodes) return kCapacityTaskGenLds;
    // Sibling to build vs subtract (exact int64 subtraction makes this
    // a performance choice only, never a correctness one):
    //  - single GPU, no monotone bounds: the DEVICE picks the
    //    smaller-row child inside HistTaskGenKernel (exact local
    //    counts) and the hist kernel accumulates its sums; the host
    //    learns the choice from the counters at the level sync.
    //  - distributed or monotone: the HOST picks by global hessian sum
    //    (rank-identical, so every rank builds/allreduces the same
    //    slot layout) and stages sums/bounds as usual.
    const bool dev_choice = (a.allreduce == nullptr) && !has_mono;
    std::vector<Node*> eval_nodes(2 * kb);  // hist slot order
    std::vector<int32_t> parent_slots;
    std::vector<int32_t> desc;  // [k][4] for HistTaskGenKernel
    desc.reserve(4 * kb);
    for (int i = 0; i < kb; ++i) {
      Node& ln = next_level[2 * i];
      Node& rn = next_level[2 * i + 1];
      parent_slots.push_back(expand[i]->hist_slot);
      desc.push_back(expand[i]->seg_begin);
      desc.push_back(expand[i]->seg_end);
      desc.push_back(i);  // counter slot
      if (dev_choice) {
        desc.push_back(2);  // device picks the smaller child
      } else {
        Node* small = (ln.hq <= rn.hq) ? &ln : &rn;
        eval_nodes[i] = small;
        eval_nodes[kb + i] = (small == &ln) ? &rn : &ln;
        desc.push_back(small == &ln ? 1 : 0);  // is_left
      }
    }

    // ---- ONE staging upload for the whole level ----
    // [partition tasks | feat | sbin | default_left | counters | desc |
    //  parent_slots | parent pair-sums]  + (device-only) ps region.
    // Counters live HERE (ring slot): partition atomics update them,
    // the task-gen kernel reads them, and the level sync reads them
    // back — no separate init copy, no persistent buffer.
    std::vector<BlockTask> ptasks;
    ChunkTasks(expand, &ptasks);
    const int slot = ring.next();
    size_t off_feat = (ptasks.size() * sizeof(BlockTask) + 7) & ~7ULL;
    size_t off_sbin = (off_feat + (size_t)kb * 4 + 7) & ~7ULL;
    size_t off_dl = (off_sbin + (size_t)kb * 4 + 7) & ~7ULL;
    size_t off_cnt = (off_dl + (size_t)kb + 7) & ~7ULL;
    size_t off_desc = (off_cnt + (size_t)kb * 8 + 7) & ~7ULL;
    size_t off_pslots = (off_desc + desc.size() * 4 + 7) & ~7ULL;
    size_t off_pps = (off_pslots + parent_slots.size() * 4 + 63) & ~63ULL;
    size_t upload_bytes =
        off_pps + (dev_choice ? (size_t)kb * 2 * sizeof(int64_t) : 0);
    size_t off_ps = (upload_bytes + 63) & ~63ULL;
    size_t total_bytes =
        off_ps + (dev_choice ? (size_t)kb * 4 * sizeof(int64_t) : 0);
    if (int e = ring.ensure(slot, total_bytes)) return e;
    char* h = (char*)ring.host[slot];
    memcpy(h, ptasks.data(), ptasks.size() * sizeof(BlockTask));
    {
      int32_t* feat = (int32_t*)(h + off_feat);
      int32_t* sbin = (int32_t*)(h + off_sbin);
      uint8_t* dl = (uint8_t*)(h + off_dl);
      int32_t* cnt = (int32_t*)(h + off_cnt);
      for (int i = 0; i < kb; ++i) {
        Node* nd = expand[i];
        feat[i] = nd->feature;
        sbin[i] = nd->bin - a.cut_ptrs_host[nd->feature];
        dl[i] = (uint8_t)nd->dir;
        cnt[2 * i] = nd->seg_begin;
        cnt[2 * i + 1] = nd->seg_end;
      }
      memcpy(h + off_desc, desc.data(), desc.size() * 4);
      memcpy(h + off_pslots, parent_slots.data(), parent_slots.size() * 4);
      if (dev_choice) {
        int64_t* pp = (int64_t*)(h + off_pps);
        for (int i = 0; i < kb; ++i) {
          pp[2 * i] = expand[i]->gq;
          pp[2 * i + 1] = expand[i]->hq;
        }
      }
    }
    HIP_CHECK(hipMemcpyAsync(ring.dev[slot], h, upload_bytes,
                             hipMemcpyHostToDevice, stream));
    char* d = (char*)ring.dev[slot];
    int32_t* cnt_dev = (int32_t*)(d + off_cnt);
    int64_t* eval_ps = dev_choice ? (int64_t*)(d + off_ps) : nullptr;
    const int64_t* parent_ps_dev =
        dev_choice ? (const int64_t*)(d + off_pps) : nullptr;

    gbt_partition(a.gidx8, a.gidx16, a.n_features, a.gidx8_col, a.gidx16_col,
                  a.n_rows, cur_ridx, alt_ridx, (const BlockTask*)d,
                  (int)ptasks.size(), (const int32_t*)(d + off_feat),
                  (const int32_t*)(d + off_sbin),
                  (const uint8_t*)(d + off_dl), nullptr, nullptr,
                  a.n_bins_feat_dev, cnt_dev, stream);
    std::swap(cur_ridx, alt_ridx);  // children now live in cur_ridx
    // host bound on the device-generated task count
    long long bound_total = 0;
    for (Node* nd : expand) bound_total += nd->seg_end - nd->seg_begin;
    int max_tasks = (int)std::min<long long>(
        std::min<long long>(bound_total / kHistMinRows, hist_tasks) + kb + 1,
        a.hist_tasks_cap);
    hipLaunchKernelGGL(HistTaskGenKernel, dim3(1), dim3(256), 0, stream,
                       cnt_dev, (const int32_t*)(d + off_desc), kb,
                       kHistMinRows, hist_tasks, max_tasks, a.hist_tasks_dev,
                       eval_ps, nullptr, nullptr, 0, nullptr);
    HIP_CHECK(hipMemsetAsync(next_pool, 0,
                             (size_t)kb * hist_row * sizeof(int64_t), stream));
    gbt_hist(a.gidx8, a.gidx16, a.n_features, a.qgpair, cur_ridx,
             a.hist_tasks_dev, max_tasks, next_pool, a.n_bins,
             a.feat_group_start_dev, a.bin_group_start_dev, a.n_groups,
             a.max_group_bins, a.cut_ptrs_dev, a.use_shared, eval_ps, stream);
    if (a.allreduce) {
      a.allreduce((long long*)next_pool, (long long)kb * hist_row);
    }
    {
      int64_t* sub_out = next_pool + (long long)kb * hist_row;
      const long long total = (long long)kb * hist_row;
      int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
      hipLaunchKernelGGL(SubtractHistKernel, dim3(blocks), dim3(256), 0,
                         stream, cur_pool, next_pool, sub_out,
                         (const int32_t*)(d + off_pslots), (int)hist_row, kb,
                         eval_ps, parent_ps_dev, nullptr);
    }
    if (int e = EvaluateEnqueue(a, sc, 2 * kb,
                                dev_choice ? nullptr : &eval_nodes, next_pool,
                                eval_ps, nullptr))
      return e;
    // ---- the ONE sync for this level ----
    const int64_t* best;
    const int32_t* cnt;
    if (int e = LevelSync(a, 2 * kb, kb, cnt_dev, &best, &cnt)) return e;
    for (int i = 0; i < kb; ++i) {
      Node& ln = next_level[2 * i];
      Node& rn = next_level[2 * i + 1];
      ln.seg_begin = expand[i]->seg_begin;
      ln.seg_end = cnt[2 * i];  // begin + n_left
      rn.seg_begin = ln.seg_end;
      rn.seg_end = expand[i]->seg_end;
      if (dev_choice) {
        // recover the device's smaller-child choice from the counters
        // (same rule as HistTaskGenKernel)
        const int nl = ln.seg_end - ln.seg_begin;
        const int nr = rn.seg_end - rn.seg_begin;
        Node* small = (nl <= nr) ? &ln : &rn;
        eval_nodes[i] = small;
        eval_nodes[kb + i] = (small == &ln) ? &rn : &ln;
      }
    }
    for (int s = 0; s < 2 * kb; ++s) {
      eval_nodes[s]->hist_slot = s;  // built 0..kb-1, subtracted kb..
      DecodeBest(best + 6 * s, eval_nodes[s]);
    }
    level_nodes.swap(next_level);
    std::swap(cur_pool, next_pool);
  }
  const int parity = (cur_ridx == a.ridx) ? 0 : 1;
  for (auto& nd : level_nodes) {
    leaves->push_back({nd.nid, nd.seg_begin, nd.seg_end, parity});
  }
  return 0;
}

// Shared epilogue: leaf values, then leaf positions — one sweep per
// ping-pong parity (a leaf's rows sit in whichever buffer was current
// when it stopped expanding).
int FinishLeaves(const GrowArgs& a, const TreeOut& out,
                 const std::vector<LeafSeg>& leaves) {
  for (int nid = 0; nid < out.n_tree_nodes; ++nid) {
    if (out.left[nid] == -1) {
      out.split_cond[nid] = (float)(out.base_weight[nid] * a.eta);
    }
  }
  PinnedRing& ring = a.ctx->ring;
  for (int par = 0; par < 2; ++par) {
    std::vector<const LeafSeg*> group;
    for (const auto& lf : leaves) {
      if (lf.parity == par) group.push_back(&lf);
    }
    if (group.empty()) continue;
    std::vector<BlockTask> tasks;
    std::vector<Node> lnodes(group.size());
    std::vector<Node*> lptrs(group.size());
    for (size_t i = 0; i < group.size(); ++i) {
      lnodes[i].seg_begin = group[i]->begin;
      lnodes[i].seg_end = group[i]->end;
      lptrs[i] = &lnodes[i];
    }
    ChunkTasks(lptrs, &tasks);
    const int slot = ring.next();
    size_t off_ids = (tasks.size() * sizeof(BlockTask) + 7) & ~7ULL;
    size_t bytes = off_ids + group.size() * sizeof(int32_t);
    if (int e = ring.ensure(slot, bytes)) return e;
    char* h = (char*)ring.host[slot];
    memcpy(h, tasks.data(), tasks.size() * sizeof(BlockTask));
    int32_t* ids = (int32_t*)(h + off_ids);
    for (size_t i = 0; i < group.size(); ++i) ids[i] = group[i]->nid;
    HIP_CHECK(hipMemcpyAsync(ring.dev[slot], h, bytes, hipMemcpyHostToDevice,
                             a.stream));
    char* d = (char*)ring.dev[slot];
    gbt_leaf_partition(par == 0 ? a.ridx : a.ridx_out, (const BlockTask*)d,
                       (int)tasks.size(), (const int32_t*)(d + off_ids),
                       a.pos_out, a.stream);
  }
  return 0;
}

}  // namespace

extern "C" {

void* gbt_driver_create() { return new DriverCtx(); }
void gbt_driver_destroy(void* ctx) { delete (DriverCtx*)ctx; }

// Test hook: run the whole-tree chain's init kernel for an n_rows root
// and compare the root hist task list it writes with ChunkTasks over the
// same root node.  Returns the number of differing tasks (0 = equal, a
// length mismatch counts), negative on a HIP error.
int gbt_root_tasks_check(long long n_rows, long long min_rows,
                         long long target_tasks, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  Node root{};
  root.seg_end = (int)n_rows;
  std::vector<Node*> nodes{&root};
  std::vector<BlockTask> want;
  ChunkTasks(nodes, &want, min_rows, target_tasks);
  const long long rpt = RootRowsPerTask(n_rows, min_rows, target_tasks);
  const int nt = RootTaskCount(n_rows, rpt);
  // layout: [0,64) scalars | [64,128) sums+maxabs in | [128,192) out |
  // tasks | row ids
  const size_t o_tasks = 192;
  const size_t o_ridx = o_tasks + (size_t)nt * sizeof(BlockTask);
  const size_t bytes = o_ridx + (size_t)std::max<long long>(n_rows, 1) * 4;
  char* d = nullptr;
  HIP_CHECK(hipMalloc((void**)&d, bytes));
  int rc = 0;
  std::vector<BlockTask> got(nt);
  hipError_t e = hipMemsetAsync(d, 0, o_tasks, stream);
  if (e == hipSuccess) {
    int32_t* sc = (int32_t*)d;
    hipLaunchKernelGGL(WtInitKernel, dim3(2), dim3(256), 0, stream,
                       (int32_t*)(d + o_ridx), n_rows, (int64_t*)nullptr,
                       0LL, sc, sc + 1, sc + 2, (BlockTask*)(d + o_tasks),
                       nt, rpt, (const int64_t*)(d + 64),
                       (const float*)(d + 80), (int64_t*)(d + 128));
    e = hipMemcpyAsync(got.data(), d + o_tasks,
                       (size_t)nt * sizeof(BlockTask), hipMemcpyDeviceToHost,
                       stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(d);
  if (e != hipSuccess) return -(int)e;
  if (want.size() != got.size()) return (int)std::max(want.size(), got.size());
  for (size_t i = 0; i < want.size(); ++i) {
    if (want[i].out_slot != got[i].out_slot ||
        want[i].row_begin != got[i].row_begin ||
        want[i].row_end != got[i].row_end)
      ++rc;
  }
  return rc;
}

// Bytes of whole-tree arena (wt_ws) that gbt_grow_tree needs for this
// configuration, monotone bound buffers included.
long long gbt_wt_arena_bytes(int max_depth, int max_nodes_level,
                             int wt_max_ptasks) {
  return (long long)MakeWtArena(max_depth, 2 * max_nodes_level, wt_max_ptasks,
                                true).total;
}

// Returns n_nodes (>0) on success, negative on failure.
int gbt_grow_tree(
    void* vctx, const uint8_t* gidx8, const uint16_t* gidx16, int n_features,
    const uint8_t* gidx8_col, const uint16_t* gidx16_col,  // feature-major
    long long n_rows, const int32_t* qgpair, const int32_t* cut_ptrs_dev,
    const float* cut_values_host, const int32_t* cut_ptrs_host,
    const int32_t* n_bins_feat_dev, const int32_t* feat_group_start_dev,
    const int32_t* bin_group_start_dev, int n_groups, int max_group_bins,
    int use_shared, int n_bins,
    // device workspace (torch-allocated)
    int32_t* ridx, int32_t* ridx_out, int64_t* hist_pool_a,
    int64_t* hist_pool_b, double* eval_gain, int32_t* eval_bin,
    uint8_t* eval_dir, int64_t* eval_lsum, int64_t* eval_best,
    int32_t* pos_out, int max_nodes_level,
    BlockTask* hist_tasks_dev,   // [hist_tasks_cap]
    int hist_tasks_cap,
    void* wt_ws,                 // whole-tree record/arg arena, or null
    long long wt_ws_bytes, int wt_max_ptasks,
    const int64_t* root_sums_dev,  // [2] exact quantized (g, h) totals
    const float* maxabs_dev,  // null, or [2] gradient max-abs: scales are
                              // derived on device for the root phase and
                              // on host after the root sync (no separate
                              // max-abs readback sync per round)
    double* out_scales,       // [2] out: the derived (g_scale, h_scale)
    // scalars
    double g_scale, double h_scale,
    double reg_lambda, double reg_alpha, double max_delta_step,
    double min_child_weight, double gamma, double eta, int max_depth,
    const int8_t* monotone_dev, const int8_t* monotone_host,
    const uint8_t* fmask_dev,  // null, or [n_features] colsample_bytree
                               // feature mask (broadcast to every node)
    AllreduceFn allreduce,
    // host tree outputs (caller-sized to 2^(max_depth+1))
    int32_t* out_left, int32_t* out_right, int32_t* out_parent,
    int32_t* out_split_index, float* out_split_cond,
    uint8_t* out_default_left,
    double* out_loss_chg,  // fp64: the grow-policy replay orders its
                           // priority queue by these exact gains
    float* out_sum_hess,
    float* out_base_weight, void* stream_v) {
  const GrowArgs a{
      (DriverCtx*)vctx, gidx8, gidx16, n_features, gidx8_col, gidx16_col,
      n_rows, qgpair, cut_ptrs_dev, cut_values_host, cut_ptrs_host,
      n_bins_feat_dev, feat_group_start_dev, bin_group_start_dev, n_groups,
      max_group_bins, use_shared, n_bins, ridx, ridx_out, hist_pool_a,
      hist_pool_b, eval_gain, eval_bin, eval_dir, eval_lsum, eval_best,
      pos_out, max_nodes_level, hist_tasks_dev, hist_tasks_cap, wt_ws,
      wt_ws_bytes, wt_max_ptasks, root_sums_dev, maxabs_dev, out_scales,
      g_scale, h_scale, reg_lambda, reg_alpha, max_delta_step,
      min_child_weight, gamma, eta, max_depth, monotone_dev, monotone_host,
      fmask_dev, allreduce, (hipStream_t)stream_v};
  TreeOut out{out_left, out_right, out_parent, out_split_index,
              out_split_cond, out_default_left, out_loss_chg, out_sum_hess,
              out_base_weight, 1};
  out.left[0] = -1;
  out.right[0] = -1;
  out.parent[0] = -1;
  const bool whole_tree = wt_ws != nullptr && maxabs_dev != nullptr &&
                          max_nodes_level <= 1024 && max_depth >= 2 &&
                          wt_max_ptasks > 0;
  std::vector<LeafSeg> leaves;
  if (int e = whole_tree ? GrowWholeTree(a, &out, &leaves)
                         : GrowPerLevel(a, &out, &leaves))
    return e;
  if (int e = FinishLeaves(a, out, leaves)) return e;
  return out.n_tree_nodes;
}

}  // extern "C"
