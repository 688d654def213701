// The front end of the 256x256-tile, 16-wave GEMM kernels gemm8.hip and
// gemm_mx8.hip: everything they do before and around their K-loops.  The
// K-loops themselves (slot layout and rotation, swizzle, the per-lane staging
// offset, fragment reads, MFMA issue, scales, schedule) are per file; the
// epilogue is tile_epilogue (mfma_tile.h).  gemm_mx4.hip has the same front
// end written out in its kernel: on this header its register allocation and
// speed changed (profiles/gemm_front_end.md).
//
// Geometry: 1024 threads = 16 waves as 4x4, 64x64 of C per wave.  Whatever
// the element type, one K-tile of an operand is 256 rows x 128 bytes, staged
// as two HALF-TILES of [128 rows][128 B] = 16 KiB: 1024 16-byte chunks, one
// per thread, so a half-tile is ONE wave-level global_load_lds (glds) per
// wave.  The two halves of a slot are adjacent in LDS.  LDS is lane-linear;
// each kernel's XOR swizzle rides on the glds SOURCE address (its stg_off)
// and on its fragment read.
//
// Landing proof (common part).  The prologue issues, in this order,
//     A0(0) A1(0) B0(0) B1(0) [B0(1) B1(1) when a second tile exists]
// and every kernel's loop issues A(T+1) before B(T+2).  Vector memory loads
// retire in issue order, so at the head of tile T `s_waitcnt vmcnt(2)` leaves
// at most the two newest in flight, and those are B(T+1)'s halves: A(T), and
// B(T), which is older still, have landed.  When no later tile exists nothing
// newer was issued and the wait is vmcnt(0).  Slot safety is the kernel's own business: what a glds overwrites
// depends on its slot rotation.
#pragma once
#include "mfma_tile.h"

#define T256_TILE 256              // rows and columns of C per block
#define T256_THREADS 1024
#define T256_HALF_BYTES (128 * 128)  // one half-tile slot

// LIVE (the fused scoring heads only): false when the block's row tile lies
// at or past the device-side live row count, else live_rows = its rows below
// the count.  Without LIVE every row is live.  The first thing a kernel does,
// ahead of any load, barrier and LDS access (live_rows.h says why); return on
// false.
template <Epi EPI, bool LIVE>
__device__ __forceinline__ bool tile256_live(
    const int64_t* __restrict__ n_live, long long M, int& live_rows) {
  live_rows = T256_TILE;
  if constexpr (LIVE) {
    static_assert(EPI == Epi::ReluDot, "live rows: scoring head only");
    return tile_live_rows<T256_TILE>(
        n_live, M, (long long)blockIdx.y * T256_TILE, live_rows);
  }
  return true;
}

// Where a thread's wave sits in the block's tile and the lane in the wave's
// fragments (mfma_tile.h's header has the C/D layout).
struct Tile256 {
  long long m0, n0;  // the block's origin in C
  int wave, lane;
  int wm, wn;        // the wave's 64x64 block: rows wm*64.., columns wn*64..
  int fl, kg;        // lane & 15, lane >> 4
};

__device__ __forceinline__ Tile256 tile256_coords() {
  Tile256 t;
  t.m0 = (long long)blockIdx.y * T256_TILE;
  t.n0 = (long long)blockIdx.x * T256_TILE;
  t.wave = threadIdx.x >> 6;
  t.lane = threadIdx.x & 63;
  t.wm = t.wave >> 2;
  t.wn = t.wave & 3;
  t.fl = t.lane & 15;
  t.kg = t.lane >> 4;
  return t;
}

__device__ __forceinline__ void zero_acc(f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
}

// Stage one half-tile: each wave's glds fills its own 1 KiB of the slot.
// off0 is the thread's source byte offset inside the half-tile (row * pitch
// + swizzled chunk), tile-invariant and 32-bit, so staging in the hot loop is
// {uniform base + int offset} with no 64-bit per-lane math.  No row clamping:
// these kernels run on whole tiles only.
__device__ __forceinline__ void tile256_stage_half(
    char* __restrict__ slot, const char* __restrict__ base, int off0) {
  const int wave = threadIdx.x >> 6;
  glds16(base + off0, slot + wave * 1024);
}

// K-tile 0 of the block's four half-tile sources: rows m0 and m0+128 of A,
// n0 and n0+128 of B; ld = storage elements (T) per operand row.
struct Tile256Src {
  const char *a0, *a1, *b0, *b1;
};

template <typename T>
__device__ __forceinline__ Tile256Src tile256_src(const T* A, const T* B,
                                                  long long m0, long long n0,
                                                  long long ld) {
  return {(const char*)(A + m0 * ld), (const char*)(A + (m0 + 128) * ld),
          (const char*)(B + n0 * ld), (const char*)(B + (n0 + 128) * ld)};
}

// Prologue: A(0) -> a_slot, B(0) -> b_slot0 and, when a second K-tile exists,
// B(1) -> b_slot1 (A(1) is the loop's first issue).  ktile_bytes: one
// K-tile along an operand row.  The issue order is part of the landing proof
// above.
__device__ __forceinline__ void tile256_prologue(
    char* a_slot, char* b_slot0, char* b_slot1, Tile256Src s,
    int stg_off, long long ktile_bytes, bool second_tile) {
  tile256_stage_half(a_slot, s.a0, stg_off);
  tile256_stage_half(a_slot + T256_HALF_BYTES, s.a1, stg_off);
  tile256_stage_half(b_slot0, s.b0, stg_off);
  tile256_stage_half(b_slot0 + T256_HALF_BYTES, s.b1, stg_off);
  if (second_tile) {
    tile256_stage_half(b_slot1, s.b0 + ktile_bytes, stg_off);
    tile256_stage_half(b_slot1 + T256_HALF_BYTES, s.b1 + ktile_bytes,
                       stg_off);
  }
}

// Head of tile T's first phase: wait until A(T) and B(T) have landed (the
// proof above); the caller's s_barrier follows.
__device__ __forceinline__ void tile256_wait_landed(bool later_tile) {
  if (later_tile)
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
