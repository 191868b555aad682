// Gradient histogram build for CDNA4 (gfx950).
//
// Reference behavior: src/tree/gpu_hist/histogram.cu StHistKernel — but
// re-designed for MI355X rather than translated:
//  - LDS-privatized per-workgroup histogram covering a whole feature
//    group (160 KiB LDS/CU lets one group hold up to ~9K bins at
//    16 B/bin; Higgs 28x256=7168 bins fits in a single group), flushed
//    to global memory once per block.
//  - 64-wide wavefronts; 512-thread blocks on the register-metadata
//    kernel (HistKernelReg), 1024 on the generic one (HistKernel).
//  - int32 quantized gradients accumulated into int64 bins via
//    atomicAdd(u64) — ds_add_u64 on LDS, global_atomic_add_u64 on HBM:
//    deterministic regardless of ordering (two's complement wraparound
//    is exact for signed fixed-point).
//  - blockIdx.x enumerates (node, row-chunk) tasks; blockIdx.y the
//    feature group, and on HistKernelReg (group, feature slice): with S
//    slices a block zeroes, accumulates and flushes only its slice's bins
//    of the group, so a row chunk's histogram is still flushed once in
//    total while the chunk is S times larger — S times fewer global
//    flush atomics at the same block count.  S comes from
//    gbt_hist_slices(); the drivers size their tasks by the same S.
#include "gbt_kernels.h"

#include <algorithm>
#include <cstdlib>

#ifndef GBT_HIST_BLOCK
#define GBT_HIST_BLOCK 1024
#endif
// slices gbt_hist_slices() returns for the measured shape class
#ifndef GBT_HIST_DEFAULT_SLICES
#define GBT_HIST_DEFAULT_SLICES 4
#endif
#define GBT_HIST_MAX_F 1024  // per-block staged feature metadata cap

template <typename BinT, bool kUseShared>
__global__ __launch_bounds__(GBT_HIST_BLOCK) void HistKernel(
    const BinT* __restrict__ gidx, int n_features,
    const int32_t* __restrict__ qgpair, const int32_t* __restrict__ ridx,
    const BlockTask* __restrict__ tasks,
    int64_t* __restrict__ out_hist, int n_bins,
    const int32_t* __restrict__ feat_group_start,
    const int32_t* __restrict__ bin_group_start,
    const int32_t* __restrict__ cut_ptrs,
    int64_t* __restrict__ node_sums /* [k,2] or null: per-slot
        gradient sums, accumulated by group-0 blocks (used by the
        1-sync native driver for device-chosen siblings) */) {
  const BlockTask task = tasks[blockIdx.x];
  // device-generated task arrays are padded with empty tasks up to the
  // launched grid (task count is not host-known in the 1-sync driver);
  // return before any LDS work — uniform across the block
  if (task.row_begin >= task.row_end) return;
  const int group = blockIdx.y;
  const int f_begin = feat_group_start[group];
  const int f_end = feat_group_start[group + 1];
  const int bin_begin = bin_group_start[group];
  const int bin_end = bin_group_start[group + 1];
  const int group_bins = bin_end - bin_begin;
  const int gf = f_end - f_begin;

  // stage per-feature (start bin - bin_begin, n_bins) in LDS so the hot
  // loop does no global cut_ptrs loads.  On the LDS path the start is
  // group-relative (< 8192) so it PACKS with the width into one 32-bit
  // word — one ds_read per (row, feature) instead of two (the hist
  // kernel is LDS-issue bound; metadata was a third of the traffic)
  __shared__ unsigned s_meta[GBT_HIST_MAX_F];   // (start << 16) | width
  __shared__ int s_start[GBT_HIST_MAX_F];       // global path (wide start)
  __shared__ int s_width[GBT_HIST_MAX_F];
  const bool stage_meta = gf <= GBT_HIST_MAX_F;
  if (stage_meta) {
    for (int f = threadIdx.x; f < gf; f += blockDim.x) {
      const int c0 = cut_ptrs[f_begin + f];
      const int wdt = cut_ptrs[f_begin + f + 1] - c0;
      if (kUseShared) {
        s_meta[f] = ((unsigned)(c0 - bin_begin) << 16) | (unsigned)wdt;
      } else {
        s_start[f] = c0;
        s_width[f] = wdt;
      }
    }
  }

  extern __shared__ unsigned long long smem[];  // [group_bins][2]
  if (kUseShared) {
    for (int i = threadIdx.x; i < group_bins * 2; i += blockDim.x) {
      smem[i] = 0ULL;
    }
  }
  __syncthreads();

  unsigned long long* hist_s = smem;
  int64_t* hist_g = out_hist + (size_t)task.out_slot * n_bins * 2;

  const bool do_sums = node_sums != nullptr && group == 0;
  long long sum_g = 0, sum_h = 0;
  for (int i = task.row_begin + (int)threadIdx.x; i < task.row_end;
       i += blockDim.x) {
    const int row = ridx[i];
    const long long g = qgpair[2 * (size_t)row];
    const long long h = qgpair[2 * (size_t)row + 1];
    if (do_sums) {
      sum_g += g;
      sum_h += h;
    }
    const BinT* rowbins = gidx + (size_t)row * n_features + f_begin;
    if (stage_meta) {
      for (int f = 0; f < gf; ++f) {
        const int local = (int)rowbins[f];
        if (kUseShared) {
          const unsigned m = s_meta[f];
          if (local >= (int)(m & 0xFFFFu)) continue;  // missing sentinel
          const int sbin = (int)(m >> 16) + local;
          atomicAdd(&hist_s[2 * sbin], (unsigned long long)g);
          atomicAdd(&hist_s[2 * sbin + 1], (unsigned long long)h);
        } else {
          if (local >= s_width[f]) continue;
          const int sbin = s_start[f] + local;
          atomicAdd((unsigned long long*)&hist_g[2 * sbin],
                    (unsigned long long)g);
          atomicAdd((unsigned long long*)&hist_g[2 * sbin + 1],
                    (unsigned long long)h);
        }
      }
    } else {
      for (int f = f_begin; f < f_end; ++f) {
        const int local = (int)rowbins[f - f_begin];
        const int c0 = cut_ptrs[f];
        if (local >= cut_ptrs[f + 1] - c0) continue;
        const int gbin = c0 + local;
        if (kUseShared) {
          const int sbin = gbin - bin_begin;
          atomicAdd(&hist_s[2 * sbin], (unsigned long long)g);
          atomicAdd(&hist_s[2 * sbin + 1], (unsigned long long)h);
        } else {
          atomicAdd((unsigned long long*)&hist_g[2 * gbin],
                    (unsigned long long)g);
          atomicAdd((unsigned long long*)&hist_g[2 * gbin + 1],
                    (unsigned long long)h);
        }
      }
    }
  }

  if (kUseShared) {
    __syncthreads();
    for (int i = threadIdx.x; i < group_bins * 2; i += blockDim.x) {
      const unsigned long long v = hist_s[i];
      if (v != 0ULL) {
        atomicAdd((unsigned long long*)&hist_g[2 * bin_begin + i], v);
      }
    }
  }
  if (do_sums) {
    for (int off = 32; off > 0; off >>= 1) {
      sum_g += __shfl_down(sum_g, off, 64);
      sum_h += __shfl_down(sum_h, off, 64);
    }
    __shared__ long long wg[GBT_HIST_BLOCK / 64];
    __shared__ long long wh[GBT_HIST_BLOCK / 64];
    const int lane = (int)threadIdx.x & 63;
    const int wave = (int)threadIdx.x >> 6;
    if (lane == 0) {
      wg[wave] = sum_g;
      wh[wave] = sum_h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long tg = 0, th = 0;
      for (int w = 0; w < (int)blockDim.x / 64; ++w) {
        tg += wg[w];
        th += wh[w];
      }
      if (tg) atomicAdd((unsigned long long*)&node_sums[2 * task.out_slot],
                        (unsigned long long)tg);
      if (th) atomicAdd(
          (unsigned long long*)&node_sums[2 * task.out_slot + 1],
          (unsigned long long)th);
    }
  }
}

// Register-metadata specialization (round-2 ladder): for a single
// feature group with few features (the Higgs-1M shape: 28 features,
// one 7168-bin LDS histogram) the generic kernel issues TWO LDS meta
// reads (s_start/s_width) per (row, feature) on top of the two
// ds_add_u64 — half the LDS issue traffic is metadata.  Here each
// thread caches the packed (start << 16 | width) metadata in
// registers once per block (kGF-bounded unrolled array), and when the
// row stride is dword-aligned the per-row bin bytes are fetched with
// packed 32-bit loads (4 features per load) instead of 28 byte loads.
// Atomic count is unchanged — this attacks the ISSUE-slot bound the
// round-1 PMC ladder identified (bank conflicts were only ~6%).
//
// Feature slices: blockIdx.y = group * slices + slice.  A group's load
// units (one 32-bit load on the kVec path, one feature otherwise) are
// cut into min(slices, units) contiguous runs as evenly as possible; a
// block owns one run: it loads only those dwords of the row and zeroes,
// accumulates and flushes only those features' bins, held in LDS
// relative to the slice's first bin.  kGF bounds the features of a
// slice (the launcher picks it from the slice count).  Blocks of a
// slice index past the group's unit count, and blocks of the grid.x
// padding (blockIdx.x >= n_tasks), return at once.
template <typename BinT, int kGF, bool kVec>
__global__ __launch_bounds__(GBT_HIST_BLOCK) void HistKernelReg(
    const BinT* __restrict__ gidx, int n_features,
    const int32_t* __restrict__ qgpair, const int32_t* __restrict__ ridx,
    const BlockTask* __restrict__ tasks,
    int64_t* __restrict__ out_hist, int n_bins,
    const int32_t* __restrict__ feat_group_start,
    const int32_t* __restrict__ cut_ptrs,
    int64_t* __restrict__ node_sums, int n_tasks, int slices) {
  if ((int)blockIdx.x >= n_tasks) return;
  const BlockTask task = tasks[blockIdx.x];
  if (task.row_begin >= task.row_end) return;
  constexpr int kLanes = kVec ? 4 / (int)sizeof(BinT) : 1;
  const int group = (int)blockIdx.y / slices;
  const int slice = (int)blockIdx.y - group * slices;
  const int f_begin = feat_group_start[group];
  const int gf = feat_group_start[group + 1] - f_begin;
  const int units = (gf + kLanes - 1) / kLanes;
  const int n_slices = min(slices, units);
  if (slice >= n_slices) return;
  // this block's features of the group: [sf_begin, sf_begin + sf)
  const int sf_begin = min(gf, slice * units / n_slices * kLanes);
  const int sf = min(
      kGF, min(gf, (slice + 1) * units / n_slices * kLanes) - sf_begin);
  const int bin_begin = cut_ptrs[f_begin + sf_begin];
  const int slice_bins = cut_ptrs[f_begin + sf_begin + sf] - bin_begin;

  unsigned meta[kGF];  // (slice-rel start << 16) | width, both < 65536
#pragma unroll
  for (int f = 0; f < kGF; ++f) {
    if (f < sf) {
      const int c0 = cut_ptrs[f_begin + sf_begin + f];
      meta[f] = ((unsigned)(c0 - bin_begin) << 16)
                | (unsigned)(cut_ptrs[f_begin + sf_begin + f + 1] - c0);
    } else {
      meta[f] = 0;
    }
  }

  extern __shared__ unsigned long long smem[];
  for (int i = threadIdx.x; i < slice_bins * 2; i += blockDim.x) {
    smem[i] = 0ULL;
  }
  __syncthreads();

  int64_t* hist_g = out_hist + (size_t)task.out_slot * n_bins * 2;
  const bool do_sums = node_sums != nullptr && blockIdx.y == 0;
  long long sum_g = 0, sum_h = 0;
  // One row in registers: its gradient pair and kW words of bins — on
  // the kVec path dword-packed loads of 4 (u8) / 2 (u16) features (the
  // launcher guarantees rows stay 4-aligned; slices begin on a load
  // unit), otherwise one feature per word.
  constexpr int kW = kGF / kLanes;
  auto load_row = [&](int row, unsigned (&w)[kW], int& g, int& h) {
    g = qgpair[2 * (size_t)row];
    h = qgpair[2 * (size_t)row + 1];
    const BinT* rowbins =
        gidx + (size_t)row * n_features + f_begin + sf_begin;
#pragma unroll
    for (int u = 0; u < kW; ++u) {
      w[u] = 0;
      if (kLanes * u < sf) {
        w[u] = kVec ? ((const unsigned*)rowbins)[u] : (unsigned)rowbins[u];
      }
    }
  };
  auto add_row = [&](const unsigned (&w)[kW], long long g, long long h) {
    if (do_sums) {
      sum_g += g;
      sum_h += h;
    }
#pragma unroll
    for (int u = 0; u < kW; ++u) {
      if (kLanes * u >= sf) break;
#pragma unroll
      for (int j = 0; j < kLanes; ++j) {
        const unsigned m = meta[kLanes * u + j];
        const int local = (int)((w[u] >> (8 * (int)sizeof(BinT) * j))
                                & (sizeof(BinT) == 1 ? 0xFFu : 0xFFFFu));
        if (local >= (int)(m & 0xFFFFu)) continue;  // missing sentinel
        const int sbin = (int)(m >> 16) + local;
        atomicAdd(&smem[2 * sbin], (unsigned long long)g);
        atomicAdd(&smem[2 * sbin + 1], (unsigned long long)h);
      }
    }
  };
  for (int i = task.row_begin + (int)threadIdx.x; i < task.row_end;
       i += blockDim.x) {
    unsigned w[kW];
    int g, h;
    load_row(ridx[i], w, g, h);
    add_row(w, g, h);
  }

  __syncthreads();
  for (int i = threadIdx.x; i < slice_bins * 2; i += blockDim.x) {
    const unsigned long long v = smem[i];
    if (v != 0ULL) {
      atomicAdd((unsigned long long*)&hist_g[2 * bin_begin + i], v);
    }
  }
  if (do_sums) {
    for (int off = 32; off > 0; off >>= 1) {
      sum_g += __shfl_down(sum_g, off, 64);
      sum_h += __shfl_down(sum_h, off, 64);
    }
    __shared__ long long wg[GBT_HIST_BLOCK / 64];
    __shared__ long long wh[GBT_HIST_BLOCK / 64];
    const int lane = (int)threadIdx.x & 63;
    const int wave = (int)threadIdx.x >> 6;
    if (lane == 0) {
      wg[wave] = sum_g;
      wh[wave] = sum_h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long tg = 0, th = 0;
      for (int w = 0; w < (int)blockDim.x / 64; ++w) {
        tg += wg[w];
        th += wh[w];
      }
      if (tg) atomicAdd((unsigned long long*)&node_sums[2 * task.out_slot],
                        (unsigned long long)tg);
      if (th) atomicAdd(
          (unsigned long long*)&node_sums[2 * task.out_slot + 1],
          (unsigned long long)th);
    }
  }
}

// Slice policy.  Measured on MI355X at one shape class only
// (profiles/r08_hist_slices.md): one LDS group of u8 bins whose flush is
// large against its row work, 28 features x 256 bins.  Everything else
// keeps one slice until it is measured.  Env GBT_HIST_SLICES overrides
// the choice for every register-kernel launch (read once per process);
// either way the result is at most the load units of the widest group.
extern "C" int gbt_hist_slices(int n_groups, int group_features,
                               int group_bins, int bin_bytes,
                               int use_shared) {
  static int env = [] {
    const char* e = getenv("GBT_HIST_SLICES");
    const int v = e ? atoi(e) : 0;
    return v >= 1 && v <= 64 ? v : 0;
  }();
  static int use_reg = [] {
    const char* e = getenv("GBT_HIST_REG");
    return e ? atoi(e) : 1;
  }();
  if (!use_reg || use_shared < 2 || (bin_bytes != 1 && bin_bytes != 2))
    return 1;
  int s = env;
  if (s == 0) {
    s = (n_groups == 1 && bin_bytes == 1 && group_features >= 16 &&
         group_features <= 32 && group_bins >= 4096)
            ? GBT_HIST_DEFAULT_SLICES : 1;
  }
  const int lanes = use_shared >= 3 ? 4 / bin_bytes : 1;
  const int gf = group_features < 32 ? group_features : 32;
  const int units = (gf + lanes - 1) / lanes;
  return s < units ? s : (units > 1 ? units : 1);
}

namespace {

template <typename BinT, bool kVec>
void LaunchHistReg(int slice_features, dim3 grid, dim3 block, size_t shmem,
                   hipStream_t stream, const BinT* gidx, int n_features,
                   const int32_t* qgpair, const int32_t* ridx,
                   const BlockTask* tasks, int64_t* out_hist, int n_bins,
                   const int32_t* feat_group_start, const int32_t* cut_ptrs,
                   int64_t* node_sums, int n_tasks, int slices) {
#define GBT_HIST_REG_LAUNCH(GF)                                              \
  hipLaunchKernelGGL((HistKernelReg<BinT, GF, kVec>), grid, block, shmem,    \
                     stream, gidx, n_features, qgpair, ridx, tasks,          \
                     out_hist, n_bins, feat_group_start, cut_ptrs,           \
                     node_sums, n_tasks, slices)
  if (slice_features <= 4) {
    GBT_HIST_REG_LAUNCH(4);
  } else if (slice_features <= 8) {
    GBT_HIST_REG_LAUNCH(8);
  } else if (slice_features <= 16) {
    GBT_HIST_REG_LAUNCH(16);
  } else {
    GBT_HIST_REG_LAUNCH(32);
  }
#undef GBT_HIST_REG_LAUNCH
}

}  // namespace

extern "C" void gbt_hist(const uint8_t* gidx8, const uint16_t* gidx16,
                         int n_features, const int32_t* qgpair,
                         const int32_t* ridx, const BlockTask* tasks,
                         int n_tasks, int64_t* out_hist, int n_bins,
                         const int32_t* feat_group_start,
                         const int32_t* bin_group_start, int n_groups,
                         int max_group_bins, const int32_t* cut_ptrs,
                         int use_shared, int64_t* node_sums,
                         hipStream_t stream) {
  const int slices = gbt_hist_slices(
      n_groups, n_groups == 1 ? n_features : 32, max_group_bins,
      gidx8 != nullptr ? 1 : 2, use_shared);
  gbt_hist_sliced(gidx8, gidx16, n_features, qgpair, ridx, tasks, n_tasks,
                  out_hist, n_bins, feat_group_start, bin_group_start,
                  n_groups, max_group_bins, cut_ptrs, use_shared, slices,
                  node_sums, stream);
}

extern "C" void gbt_hist_sliced(
    const uint8_t* gidx8, const uint16_t* gidx16, int n_features,
    const int32_t* qgpair, const int32_t* ridx, const BlockTask* tasks,
    int n_tasks, int64_t* out_hist, int n_bins,
    const int32_t* feat_group_start, const int32_t* bin_group_start,
    int n_groups, int max_group_bins, const int32_t* cut_ptrs, int use_shared,
    int slices, int64_t* node_sums, hipStream_t stream) {
  static int block_env = [] {
    const char* e = getenv("GBT_HIST_BLOCK_SIZE");
    int v = e ? atoi(e) : 0;
    return (v >= 64 && v <= 1024) ? (v & ~63) : 0;
  }();
  const int block_size = block_env ? block_env : GBT_HIST_BLOCK;
  // round-2 sweep: the register-metadata kernel peaks at 512 threads
  // (972 vs 918 rounds/s at 1024 — fewer waves contending the LDS
  // atomic pipe, still enough to hide ds latency)
  const int reg_block = block_env ? block_env : 512;
  dim3 grid(n_tasks, n_groups);
  dim3 block(block_size);
  size_t shmem = use_shared ? (size_t)max_group_bins * 2 * sizeof(int64_t) : 0;
  // register-metadata fast path (HistKernelReg): selected by the
  // CALLER through use_shared (it owns the host-side group geometry):
  //   0 = global-atomic fallback, 1 = generic LDS kernel,
  //   2 = register-metadata (every group <= 32 features, u8),
  //   3 = 2 + dword-packed bin loads (stride/group 4-aligned).
  // Env GBT_HIST_REG=0 forces the generic kernel for A/B.
  static int use_reg = [] {
    const char* e = getenv("GBT_HIST_REG");
    return e ? atoi(e) : 1;
  }();
  if (use_reg && use_shared >= 2) {
    // host-side bounds of the slice geometry the kernel derives per
    // group: a group has at most max_gf features, so at most units_max
    // load units, and an even cut into s runs gives runs of at most
    // ceil(units_max / s) units
    const int lanes = use_shared >= 3 ? (gidx8 != nullptr ? 4 : 2) : 1;
    const int max_gf = std::min(n_groups == 1 ? n_features : 32, 32);
    const int units_max = (max_gf + lanes - 1) / lanes;
    const int s = std::max(1, std::min(slices, units_max));
    // one slice is the unsliced launch: kGF = 32, the group's bins
    const int slice_features = s == 1 ? 32 : (units_max + s - 1) / s * lanes;
    dim3 rgrid(n_tasks, n_groups);
    if (s > 1) {
      // Workgroups go to the 8 XCDs round-robin in linear id order
      // (x fastest).  With grid.x a multiple of 8, block (x, y) lands
      // on XCD x % 8 for every y: the slices of one row chunk share an
      // L2, so the chunk's rows are fetched from HBM once.  Env
      // GBT_HIST_XCD_ALIGN=0 drops the padding for A/B.
      static int xcd_align = [] {
        const char* e = getenv("GBT_HIST_XCD_ALIGN");
        return e ? atoi(e) : 1;
      }();
      rgrid = dim3(xcd_align ? (n_tasks + 7) / 8 * 8 : n_tasks,
                   n_groups * s);
      // a u8 feature has at most 256 bins (its local ids and the
      // missing sentinel fit a byte), which bounds a slice's bins
      // without the host knowing the cuts; u16 keeps the group's size
      // (sized by the kGF LaunchHistReg picks, which caps the kernel's
      // slice)
      if (gidx8 != nullptr) {
        const int kgf = slice_features <= 4 ? 4 : slice_features <= 8 ? 8
                        : slice_features <= 16 ? 16 : 32;
        shmem = (size_t)std::min(max_group_bins, kgf * 256) * 2 *
                sizeof(int64_t);
      }
    }
    dim3 rblock(reg_block);
    if (gidx8 != nullptr) {
      if (use_shared >= 3) {
        LaunchHistReg<uint8_t, true>(slice_features, rgrid, rblock, shmem,
                                     stream, gidx8, n_features, qgpair, ridx,
                                     tasks, out_hist, n_bins,
                                     feat_group_start, cut_ptrs, node_sums,
                                     n_tasks, s);
      } else {
        LaunchHistReg<uint8_t, false>(slice_features, rgrid, rblock, shmem,
                                      stream, gidx8, n_features, qgpair, ridx,
                                      tasks, out_hist, n_bins,
                                      feat_group_start, cut_ptrs, node_sums,
                                      n_tasks, s);
      }
    } else {
      if (use_shared >= 3) {
        LaunchHistReg<uint16_t, true>(slice_features, rgrid, rblock, shmem,
                                      stream, gidx16, n_features, qgpair,
                                      ridx, tasks, out_hist, n_bins,
                                      feat_group_start, cut_ptrs, node_sums,
                                      n_tasks, s);
      } else {
        LaunchHistReg<uint16_t, false>(slice_features, rgrid, rblock, shmem,
                                       stream, gidx16, n_features, qgpair,
                                       ridx, tasks, out_hist, n_bins,
                                       feat_group_start, cut_ptrs, node_sums,
                                       n_tasks, s);
      }
    }
    return;
  }
  if (gidx8 != nullptr) {
    if (use_shared) {
      hipLaunchKernelGGL((HistKernel<uint8_t, true>), grid, block, shmem,
                         stream, gidx8, n_features, qgpair, ridx, tasks,
                         out_hist, n_bins, feat_group_start, bin_group_start,
                         cut_ptrs, node_sums);
    } else {
      hipLaunchKernelGGL((HistKernel<uint8_t, false>), grid, block, 0, stream,
                         gidx8, n_features, qgpair, ridx, tasks, out_hist,
                         n_bins, feat_group_start, bin_group_start, cut_ptrs,
                         node_sums);
    }
  } else {
    if (use_shared) {
      hipLaunchKernelGGL((HistKernel<uint16_t, true>), grid, block, shmem,
                         stream, gidx16, n_features, qgpair, ridx, tasks,
                         out_hist, n_bins, feat_group_start, bin_group_start,
                         cut_ptrs, node_sums);
    } else {
      hipLaunchKernelGGL((HistKernel<uint16_t, false>), grid, block, 0, stream,
                         gidx16, n_features, qgpair, ridx, tasks, out_hist,
                         n_bins, feat_group_start, bin_group_start, cut_ptrs,
                         node_sums);
    }
  }
}

// Fused multi-target histogram (reference MtHistKernel,
// src/tree/gpu_hist/histogram.cu:256): ONE pass over the rows
// accumulates every target's (g, h) — the python fallback launches the
// single-target kernel T times and re-reads the bin matrix per target.
// LDS layout [group_bins][T][2] u64; the caller regroups features so
// T * group_bins * 16 B fits the LDS budget.  Output is target-major:
// out[slot][T][n_bins][2] (the MT grower's stacked-tensor layout).
#define GBT_HIST_MT_MAX_T 8

template <typename BinT>
__global__ __launch_bounds__(512) void HistMtKernel(
    const BinT* __restrict__ gidx, int n_features,
    const int32_t* __restrict__ qg /* [n][T][2] */, int T,
    const int32_t* __restrict__ ridx, const BlockTask* __restrict__ tasks,
    int64_t* __restrict__ out_hist /* [T][n_slots][n_bins][2] */,
    int n_bins, int n_slots,
    const int32_t* __restrict__ feat_group_start,
    const int32_t* __restrict__ bin_group_start,
    const int32_t* __restrict__ cut_ptrs) {
  const BlockTask task = tasks[blockIdx.x];
  if (task.row_begin >= task.row_end) return;
  const int group = blockIdx.y;
  const int f_begin = feat_group_start[group];
  const int f_end = feat_group_start[group + 1];
  const int bin_begin = bin_group_start[group];
  const int group_bins = bin_group_start[group + 1] - bin_begin;
  const int gf = f_end - f_begin;

  __shared__ int s_start[GBT_HIST_MAX_F];
  __shared__ int s_width[GBT_HIST_MAX_F];
  for (int f = threadIdx.x; f < gf; f += blockDim.x) {
    const int c0 = cut_ptrs[f_begin + f];
    s_start[f] = c0 - bin_begin;
    s_width[f] = cut_ptrs[f_begin + f + 1] - c0;
  }
  extern __shared__ unsigned long long smem[];  // [group_bins][T][2]
  const int total = group_bins * T * 2;
  for (int i = threadIdx.x; i < total; i += blockDim.x) smem[i] = 0ULL;
  __syncthreads();

  for (int i = task.row_begin + (int)threadIdx.x; i < task.row_end;
       i += blockDim.x) {
    const int row = ridx[i];
    long long gv[GBT_HIST_MT_MAX_T], hv[GBT_HIST_MT_MAX_T];
    const int32_t* qp = qg + (size_t)row * T * 2;
    for (int t = 0; t < T; ++t) {
      gv[t] = qp[2 * t];
      hv[t] = qp[2 * t + 1];
    }
    const BinT* rowbins = gidx + (size_t)row * n_features + f_begin;
    for (int f = 0; f < gf; ++f) {
      const int local = (int)rowbins[f];
      if (local >= s_width[f]) continue;
      unsigned long long* cell =
          smem + ((size_t)(s_start[f] + local) * T) * 2;
      for (int t = 0; t < T; ++t) {
        atomicAdd(&cell[2 * t], (unsigned long long)gv[t]);
        atomicAdd(&cell[2 * t + 1], (unsigned long long)hv[t]);
      }
    }
  }
  __syncthreads();
  // flush [bin][t][c] -> out[slot][t][bin_begin+bin][c]
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const unsigned long long v = smem[i];
    if (v == 0ULL) continue;
    const int c = i & 1;
    const int t = (i >> 1) % T;
    const int bin = (i >> 1) / T;
    atomicAdd((unsigned long long*)&out_hist[
                  (((size_t)t * n_slots + task.out_slot) * n_bins
                   + bin_begin + bin) * 2 + c], v);
  }
}

extern "C" void gbt_hist_mt(const uint8_t* gidx8, const uint16_t* gidx16,
                            int n_features, const int32_t* qg, int T,
                            const int32_t* ridx, const BlockTask* tasks,
                            int n_tasks, int64_t* out_hist, int n_bins,
                            int n_slots,
                            const int32_t* feat_group_start,
                            const int32_t* bin_group_start, int n_groups,
                            int max_group_bins, const int32_t* cut_ptrs,
                            hipStream_t stream) {
  dim3 grid(n_tasks, n_groups);
  dim3 block(512);
  size_t shmem = (size_t)max_group_bins * T * 2 * sizeof(int64_t);
  if (gidx8 != nullptr) {
    hipLaunchKernelGGL((HistMtKernel<uint8_t>), grid, block, shmem, stream,
                       gidx8, n_features, qg, T, ridx, tasks, out_hist,
                       n_bins, n_slots, feat_group_start, bin_group_start,
                       cut_ptrs);
  } else {
    hipLaunchKernelGGL((HistMtKernel<uint16_t>), grid, block, shmem, stream,
                       gidx16, n_features, qg, T, ridx, tasks, out_hist,
                       n_bins, n_slots, feat_group_start, bin_group_start,
                       cut_ptrs);
  }
}
