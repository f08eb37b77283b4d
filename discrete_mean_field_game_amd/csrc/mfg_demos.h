// Demonstrations from agent logs (mfg_demos_from_logs, include/mfg_hip.h): states and actions counted from topic [N, H, U].
//   k_demos_keys    grid (chunks x rows) x 256: the category histogram the ranking sorts by -- hour 0 of every day
//                   (MFG_DEMOS_ORDER_FIRST_HOUR, a row per day) or every hour of every day into ONE row (MFG_DEMOS_ORDER_TOTAL).
//                   One C-bin tile in LDS per workgroup, a 64-bit global atomic per non-zero bin.  Not launched for a given order.
//   k_demos_rank    a workgroup per day x 1 024: rank[c] = #{c' : key[c'] > key[c], or equal and c' < c} from keys in LDS
//                   (one workgroup in all for MFG_DEMOS_ORDER_TOTAL, which writes every day's row), or the given table checked;
//                   writes the rank table of the workspace and `order`.
//   k_demos_count   grid (groups x days) x 256: a workgroup owns every groups-th chunk of MFG_DEMOS_CHUNK agents of one day and
//                   walks a chunk's hours with the previous hour's ranks packed four to a register.  (width + 1)^2 tiles in
//                   LDS, one per transition of a block of hours (all of them when they fit: the log is read once), row /
//                   column `width` standing for absent: counts are the tile's row sums (and, for the last hour, its column
//                   sums), so one LDS update per agent and hour serves both tables.  Flushed once per block of hours.
//   k_demos_finish  a workgroup per (day, hour) x 256: steps 5 to 7 of the header from the integer tables.
// Workspace: [keys int64 [N, C] | rank int32 [N, C] | counts int32 [N, H, width] | moves int32 [N, H-1, width, width]], each
// section rounded up to 256 bytes; zeroed on the stream before the first launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"

namespace mfg {

constexpr int DEMOS_THREADS = 256;
constexpr int DEMOS_WAVES = DEMOS_THREADS / 64;
constexpr int DEMOS_SLOTS = MFG_DEMOS_CHUNK / DEMOS_THREADS;   // agents of one thread per hour: 32, eight 16-byte loads
constexpr int DEMOS_RANK_THREADS = 1024;
constexpr int DEMOS_MAX_WIDTH = 64;
constexpr int DEMOS_LDS_BUDGET = 64 * 1024;

struct DemosWs {
  unsigned long long* keys;
  int32_t* rank;
  int32_t* counts;
  int32_t* moves;
  size_t bytes;
};

inline size_t demos_up(size_t b) { return (b + 255) / 256 * 256; }

inline DemosWs demos_layout(void* base, int N, int H, int C, int width) {
  char* p = reinterpret_cast<char*>(base);
  DemosWs w;
  size_t at = 0;
  w.keys = reinterpret_cast<unsigned long long*>(p + at), at += demos_up((size_t)N * C * 8);
  w.rank = reinterpret_cast<int32_t*>(p + at), at += demos_up((size_t)N * C * 4);
  w.counts = reinterpret_cast<int32_t*>(p + at), at += demos_up((size_t)N * H * width * 4);
  w.moves = reinterpret_cast<int32_t*>(p + at), at += demos_up((size_t)N * (H - 1) * width * width * 4);
  w.bytes = at;
  return w;
}

// The LDS of k_demos_count: `hours` transitions' (width + 1)^2 tiles next to the day's rank bytes -- all H - 1 when they fit,
// three at width = 64 --, then as many copies of them as fit, one per wave at most (two at width = 20, H = 16).
struct DemosTiles {
  int hours, copies;
  size_t lds_bytes;
};

inline DemosTiles demos_tiles(int H, int C, int width) {
  const int tile = (width + 1) * (width + 1) * 4, ranks = (C + 3) / 4 * 4, room = DEMOS_LDS_BUDGET - ranks;
  DemosTiles t;
  t.hours = room / tile < H - 1 ? room / tile : H - 1;
  t.copies = room / (t.hours * tile) < DEMOS_WAVES ? room / (t.hours * tile) : DEMOS_WAVES;
  t.lds_bytes = (size_t)t.copies * t.hours * tile + ranks;
  return t;
}

// The chunk's values of one hour: slot s of a thread.  VEC (U a multiple of 4, the log 16-byte aligned): eight 16-byte loads,
// slot s is agent (s / 4) 1 024 + 4 tid + s % 4 of the chunk; else 32 coalesced 4-byte loads, slot s is agent 256 s + tid.
// Agents past U read as -1: absent.
template <bool VEC>
__device__ __forceinline__ void demos_load(const int32_t* __restrict__ row, int64_t left, int32_t (&v)[DEMOS_SLOTS]) {
  const int tid = threadIdx.x;
  if (VEC) {
#pragma unroll
    for (int r = 0; r < DEMOS_SLOTS / 4; ++r) {
      const int off = r * (DEMOS_THREADS * 4) + tid * 4;
      int4 q = make_int4(-1, -1, -1, -1);
      if (off < left) q = *reinterpret_cast<const int4*>(row + off);
      v[4 * r] = q.x, v[4 * r + 1] = q.y, v[4 * r + 2] = q.z, v[4 * r + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < DEMOS_SLOTS; ++s) {
      const int off = s * DEMOS_THREADS + tid;
      v[s] = off < left ? row[off] : -1;
    }
  }
}

// ranks of one hour of a chunk, packed four to a register; true when a value >= C was seen
template <bool VEC>
__device__ __forceinline__ bool demos_ranks(const int32_t* __restrict__ row, int64_t left, const uint8_t* rk, int C, int width,
                                            int32_t (&cur)[DEMOS_SLOTS]) {
  demos_load<VEC>(row, left, cur);
  bool bad = false;
#pragma unroll
  for (int s = 0; s < DEMOS_SLOTS; ++s) {
    const int v = cur[s];
    bad = bad || v >= C;
    cur[s] = (v >= 0 && v < C) ? rk[v] : width;                          // `width`: absent
  }
  return bad;
}

void launch_demos(const mfg_demos_t& f, hipStream_t st);

}  // namespace mfg
