// MXFP4 (OCP e2m1 codes, per-32-element E8M0 block scales) 256x256-tile NT
// GEMM for gfx950, its two quantisers and the fused scoring head — the
// opt-in 4-bit scoring path.
//
// The instruction is the one gemm_mx8.hip runs,
// __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4, in its fp4 form (cbsz =
// blgp = 4): a lane's operand is 4 VGPRs = 32 consecutive K elements, half
// the MFMA passes and half the LDS bytes per K of the fp8 form.  A 3-bit
// magnitude cannot live on one per-tensor exponent, so every 32-element block
// carries its own scale and the K-loop has scale traffic, which the fp8
// kernel never had.  That makes this K-loop a design of its own:
//
// Geometry (what tile_epilogue assumes): 16 waves (4x4) per 1024-thread
// block, 64x64 of C per wave = 4x4 fragments of 16x16.
//
// K-tile = 256 elements = 128 B per row, so a half-tile is gemm_mx8's
// 16 KiB [128 rows][128 B], staged by ONE wave-level global_load_lds per
// wave.  One K-tile is TWO K=128 MFMAs per output fragment (h = 0, 1); MFMA
// h of lane (fl = lane&15, kg = lane>>4) takes the 16-byte chunk 4h+kg of
// its row: one ds_read_b128.  The XOR swizzle is at that 16-byte
// granularity: chunk c of row r lives at chunk position c ^ ((r>>1) & 7), so
// the 16 rows a b128 read touches at one kg cover all 64 banks (r&1 picks
// the 128-byte half of the bank space, (r>>1)&7 the chunk within it).  The
// swizzle is carried on the glds SOURCE address, as in the other kernels.
//
// Registers: the tile is consumed as two K=128 sub-steps, each holding 4 B
// fragments (16 VGPRs) and 2 A fragments (8 VGPRs) beside the 64
// accumulators and 8 scale VGPRs — less than the fp8 kernel, which holds
// 8-VGPR fragments.
//
// Scales: global -> VGPR, no LDS (the five tile slots fill all 160 KB).
// Per K-tile a wave needs 64 rows x 8 blocks = 512 scale bytes for A and as
// many for B.  The quantisers write them pre-shuffled (mx4_scale_index,
// expand1d.h) so that is ONE 8-byte load per lane per operand: dword h is
// the scale VGPR of MFMA h, byte i of it the scale of fragment i, picked by
// the MFMA's constant op_sel.  Each lane's byte scales exactly the 32
// elements that lane supplies (row fl, block 4h+kg).  They are fetched one
// tile ahead.
//
// Schedule (A double-, B triple-buffered, one barrier per K-tile; slots A
// T%2, B T%3).  Per tile T:
//
//   wait vmcnt(2) [vmcnt(0) on the last tile]; barrier
//   load scales S(T+1) -> VGPR
//   issue A(T+1) -> slot (T+1)%2   [overwrites A(T-1), read last phase]
//   issue B(T+2) -> slot (T+2)%3   [overwrites B(T-1), read last phase]
//   h = 0, 1: read B x4 + A frag 0,1; 8 MFMAs; read A frag 2,3; 8 MFMAs
//
// Landing proof: vector memory loads (glds and plain) retire in issue
// order, so vmcnt(2) leaves at most the two NEWEST of them in flight.  In
// program order the newest two at wait(T) are B(T+1)'s halves, issued at
// phase T-1 after S(T) and A(T); B(T) is older still (phase T-2).  So A(T),
// B(T) and S(T) have landed.  The proof does not lean on where the compiler
// places the scale loads: a plain load scheduled anywhere else only pushes
// more glds out of the newest two, i.e. the wait can only cover MORE tile
// loads, never fewer (the cost would be B's extra tile of slack, not
// correctness).  The scale loads are asm (see the K-loop), so this wait is
// the only one they have; no load is in flight when the kernel reaches its
// epilogue.  Near the end the guarded issues only shrink the outstanding
// set and the last tile waits vmcnt(0).
// Slot safety: both overwrites target buffers whose reads fed the PREVIOUS
// phase's MFMAs, before this phase's barrier.  Slot rotation is on pointer
// variables, never on unrolled indices.
//
// Live rows (scoring head): tile_live_rows runs before any load, barrier or
// LDS access.  A partly live tile computes its dead rows from whatever their
// codes and scales hold; a row of A reaches only its own row of C (its scale
// too), and the epilogue drops dead rows.
//
// Numerics contract (ops/reference.py states the same rule): codes 0..7 are
// 0, 0.5, 1, 1.5, 2, 3, 4, 6, bit 3 the sign; two codes per byte along K,
// element 2i in the low nibble; block exponent e = smallest integer with
// amax / 2^e <= 6, from the float's fields; round to nearest, ties to the
// even code, saturating at +-6.  C accumulates in fp32 in the MFMA.
// A block that holds an inf or a NaN has e = 0 and its finite elements are
// quantised at that e; inf saturates to +-6, and a NaN element becomes code 7
// with the NaN's own sign bit (+-6, what the packed convert emits for it,
// whatever its payload; e2m1 has no NaN).  Scale bytes 0..254 are exact
// through the MFMA, alone and in pairs (2^-127 against 2^127 in one
// product); byte 255 is NaN and is only ever met on dead rows.
//
// This kernel keeps its own copy of the front end that gemm8.hip and
// gemm_mx8.hip take from tile256.h: built on that header it allocated 126
// VGPRs instead of 118 and its scoring head measured 0.6% slower
// (profiles/gemm_front_end.md).  The host side is gemm_host.h's.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "bf16_utils.h"
#include "expand1d.h"
#include "gemm_host.h"
#include "mfma_tile.h"

#define M4_BM 256
#define M4_BN 256
#define M4_BK 256            // fp4 elements per K-tile (128 bytes/row)
#define M4_ROWB 128          // bytes per row of a K-tile
#define M4_THREADS 1024
#define M4_HTB (128 * 128)   // bytes per half-tile slot
#define M4_FMT 4             // the scaled MFMA's cbsz / blgp value for fp4
#define M4_SCHUNK 512        // scale bytes per (64-row group, K-tile)

typedef __attribute__((ext_vector_type(8))) int m4_i32x8;
typedef __attribute__((ext_vector_type(4))) int m4_i32x4;
typedef __attribute__((ext_vector_type(2))) int m4_i32x2;

// the builtin takes 8 dwords whatever the format; fp4 reads the low four
__device__ __forceinline__ m4_i32x8 m4_operand(m4_i32x4 v) {
  return __builtin_shufflevector(v, v, 0, 1, 2, 3, -1, -1, -1, -1);
}

// stage one [128 rows][128 B] half-tile: 1024 16-B chunks, 1024 threads
__device__ __forceinline__ void m4_stage_half(char* __restrict__ slot,
                                              const char* __restrict__ base,
                                              int off0) {
  const int wave = threadIdx.x >> 6;
  glds16(base + off0, slot + wave * 1024);
}

// ---- quantiser: x [R, K] -> (codes [R, K/2], scales) -----------------------
template <typename T>
__global__ void quantize_mxfp4_kernel(const T* __restrict__ x,
                                      unsigned char* __restrict__ q,
                                      unsigned char* __restrict__ s,
                                      long long R, int k8 /* K/8 */) {
  e1d_for_each_chunk(R, k8, [&](long long row, int c8) {
    float v[8];
    const long long o = e1d_offset(row, k8, c8);
    if constexpr (sizeof(T) == 2) {
      bf16x8_to_f32(load_bf16x8((const bf16_t*)x + o), v);
    } else {
      const float4 lo = *(const float4*)((const float*)x + o);
      const float4 hi = *(const float4*)((const float*)x + o + 4);
      v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w;
      v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    }
    e1d_store_mxfp4(q, s, row, k8, c8, v);
  });
}

// ---- fused rank-1 expand -> MXFP4 ------------------------------------------
//
// The fp4 scoring forward's layer 1: h1 = relu(x*w + b) emitted directly as
// codes and block scales (0.53 HBM bytes per element), the twin of
// expand1d_e4m3_kernel.  It quantises the fp32 fmaf value.
template <bool HAS_BIAS>
__global__ void expand1d_mxfp4_kernel(const float* __restrict__ x,
                                      const bf16_t* __restrict__ w,
                                      const bf16_t* __restrict__ b,
                                      unsigned char* __restrict__ q,
                                      unsigned char* __restrict__ s,
                                      long long n, int h8 /* H/8 */,
                                      const int64_t* __restrict__ n_live) {
  // rows at or past the live count are neither read nor written
  if (n_live != nullptr) n = live_count(n_live, n);
  e1d_for_each_chunk(n, h8, [&](long long row, int c8) {
    float acc[8];
    e1d_axpb<true, HAS_BIAS>(x[row], w, b, c8, acc);
    e1d_store_mxfp4(q, s, row, h8, c8, acc);
  });
}

// ---- the GEMM kernel -------------------------------------------------------
//
// Schedule, landing proof and slot safety: see the file header.
template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool LIVE = false>
__launch_bounds__(M4_THREADS)
__global__ void gemm_mxfp4_nt_kernel(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ SA,
    const unsigned char* __restrict__ B, const unsigned char* __restrict__ SB,
    const float* __restrict__ bias, const float* __restrict__ w3,
    void* __restrict__ C, long long M, long long N, long long K,
    const int64_t* __restrict__ n_live = nullptr) {  // LIVE only
  __shared__ char lds[10 * M4_HTB];  // A 2 slots + B 3 slots, 160 KB
  const long long m0 = (long long)blockIdx.y * M4_BM;
  int live_rows = M4_BM;
  if constexpr (LIVE) {
    static_assert(EPI == Epi::ReluDot, "live rows: scoring head only");
    if (!tile_live_rows<M4_BM>(n_live, M, m0, live_rows)) return;
  }
  const long long n0 = (long long)blockIdx.x * M4_BN;
  // wave-uniform by construction; telling the compiler keeps what derives
  // from it (scale chunk pointers, half-tile read bases) in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 2;
  const int wn = wave & 3;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  const int nt = (int)(K / M4_BK);
  const long long Kb = K >> 1;  // bytes per operand row

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // slots rotate as plain pointers (they only ever shape LDS addresses)
  char* aw0 = lds;                // holds A(T) at even T
  char* aw1 = lds + 2 * M4_HTB;   // holds A(T) at odd T
  char* bw0 = lds + 4 * M4_HTB;   // holds B(T)
  char* bw1 = lds + 6 * M4_HTB;   // holds B(T+1)
  char* bw2 = lds + 8 * M4_HTB;   // staging target for B(T+2)

  // this lane's read offset inside a half-tile for MFMA 0; MFMA 1 reads
  // chunk c+4, whose swizzled position is this one with bit 6 flipped
  const int rd0 = fl * M4_ROWB + (((kg ^ (fl >> 1)) & 7) * 16);
  const int a_rd = (wm >> 1) * M4_HTB + (wm & 1) * 64 * M4_ROWB + rd0;
  const int b_rd = (wn >> 1) * M4_HTB + (wn & 1) * 64 * M4_ROWB + rd0;

  // staging source offset (tile-invariant): thread ci fills LDS chunk
  // position ci&7 of row ci>>3, which holds source chunk pos ^ ((row>>1)&7)
  int stg_off;
  {
    const int ci = (int)threadIdx.x;
    const int row = ci >> 3;
    const int c16 = (ci & 7) ^ ((row >> 1) & 7);
    stg_off = (int)(row * Kb + c16 * 16);
  }
  const char* Ah0 = (const char*)(A + m0 * Kb);
  const char* Ah1 = (const char*)(A + (m0 + 128) * Kb);
  const char* Bh0 = (const char*)(B + n0 * Kb);
  const char* Bh1 = (const char*)(B + (n0 + 128) * Kb);
  // this wave's 64 rows are one scale group: chunk t of it, 8 bytes a lane
  const unsigned char* sa_p = SA + ((m0 >> 6) + wm) * (long long)nt * M4_SCHUNK;
  const unsigned char* sb_p = SB + ((n0 >> 6) + wn) * (long long)nt * M4_SCHUNK;
  const unsigned int s_lane = (unsigned int)lane * 8u;

  // prologue: S(0), then A(0), B(0), B(1).  The scale VGPRs ping-pong
  // between two named pairs (even tiles s?0, odd tiles s?1): a "next ->
  // current" copy at the end of a phase would make the compiler wait for
  // the prefetched scales, and with them for every tile load, each phase.
  //
  // The loads are written as asm: the compiler, where it tracks a pending
  // VGPR load next to in-flight glds, waits vmcnt(0) at the first use (seen
  // in the ISA), which would drain every tile load each trip.  Their landing
  // is covered by the phase's own vmcnt wait (file header); M4_SCALES_LANDED
  // after that wait is the point from which the registers may be read.
#define M4_LOAD_SCALES(dst, base)                                           \
  asm volatile("global_load_dwordx2 %0, %1, %2"                             \
               : "=&v"(dst)                                                 \
               : "v"(s_lane), "s"(base)                                     \
               : "memory")
#define M4_SCALES_LANDED(sa, sb) asm volatile("" : "+v"(sa), "+v"(sb))
  m4_i32x2 sa0, sb0, sa1 = {0, 0}, sb1 = {0, 0};
  M4_LOAD_SCALES(sa0, sa_p);
  M4_LOAD_SCALES(sb0, sb_p);
  m4_stage_half(aw0, Ah0, stg_off);
  m4_stage_half(aw0 + M4_HTB, Ah1, stg_off);
  m4_stage_half(bw0, Bh0, stg_off);
  m4_stage_half(bw0 + M4_HTB, Bh1, stg_off);
  if (nt > 1) {
    m4_stage_half(bw1, Bh0 + M4_ROWB, stg_off);
    m4_stage_half(bw1 + M4_HTB, Bh1 + M4_ROWB, stg_off);
  }

  m4_i32x4 b_f[4];
  m4_i32x4 a_f[2];

  // fragment f (16 rows) of this wave's 64, K=128 half h of the tile
#define M4_READ(dst, slot, rd, f, h)                                        \
  dst = *(const m4_i32x4*)((slot) + ((rd) ^ ((h) * 64)) + (f) * 16 * M4_ROWB)
  // op_sel must be a literal: fragment i picks byte i of the A scale VGPR,
  // column fragment nf byte nf of the B scale VGPR
#define M4_MFMA1(i, nf, af, sav, sbv)                                       \
  acc[i][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(            \
      m4_operand(af), m4_operand(b_f[nf]), acc[i][nf], M4_FMT, M4_FMT, i,   \
      sav, nf, sbv)
#define M4_MFMA(i, af, sav, sbv)                                            \
  do {                                                                      \
    M4_MFMA1(i, 0, af, sav, sbv);                                           \
    M4_MFMA1(i, 1, af, sav, sbv);                                           \
    M4_MFMA1(i, 2, af, sav, sbv);                                           \
    M4_MFMA1(i, 3, af, sav, sbv);                                           \
  } while (0)
#define M4_SUBSTEP(h, aslot, bslot, sav, sbv)                               \
  do {                                                                      \
    M4_READ(b_f[0], bslot, b_rd, 0, h);                                     \
    M4_READ(b_f[1], bslot, b_rd, 1, h);                                     \
    M4_READ(b_f[2], bslot, b_rd, 2, h);                                     \
    M4_READ(b_f[3], bslot, b_rd, 3, h);                                     \
    M4_READ(a_f[0], aslot, a_rd, 0, h);                                     \
    M4_READ(a_f[1], aslot, a_rd, 1, h);                                     \
    __builtin_amdgcn_s_setprio(1);                                          \
    M4_MFMA(0, a_f[0], sav[h], sbv[h]);                                     \
    M4_MFMA(1, a_f[1], sav[h], sbv[h]);                                     \
    __builtin_amdgcn_s_setprio(0);                                          \
    M4_READ(a_f[0], aslot, a_rd, 2, h);                                     \
    M4_READ(a_f[1], aslot, a_rd, 3, h);                                     \
    __builtin_amdgcn_s_setprio(1);                                          \
    M4_MFMA(2, a_f[0], sav[h], sbv[h]);                                     \
    M4_MFMA(3, a_f[1], sav[h], sbv[h]);                                     \
    __builtin_amdgcn_s_setprio(0);                                          \
  } while (0)
  // One phase = tile T: A(T) in acur, B(T) in brd, scales in (sac, sbc).
  // g1: tile T+1 exists (fetch its scales into (san, sbn), stage A(T+1) into
  // anxt); g2: tile T+2 exists (stage B(T+2) into bst).
#define M4_PHASE(T, acur, anxt, brd, bst, sac, sbc, san, sbn, g1, g2)       \
  do {                                                                      \
    if (g1)                                                                 \
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                      \
    else                                                                    \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      \
    M4_SCALES_LANDED(sac, sbc);                                             \
    __builtin_amdgcn_s_barrier();                                           \
    if (g1) {                                                               \
      const long long so = (long long)((T) + 1) * M4_SCHUNK;                \
      M4_LOAD_SCALES(san, sa_p + so);                                       \
      M4_LOAD_SCALES(sbn, sb_p + so);                                       \
      const long long ko = (long long)((T) + 1) * M4_ROWB;                  \
      m4_stage_half(anxt, Ah0 + ko, stg_off);                               \
      m4_stage_half(anxt + M4_HTB, Ah1 + ko, stg_off);                      \
    }                                                                       \
    if (g2) {                                                               \
      const long long ko = (long long)((T) + 2) * M4_ROWB;                  \
      m4_stage_half(bst, Bh0 + ko, stg_off);                                \
      m4_stage_half(bst + M4_HTB, Bh1 + ko, stg_off);                       \
    }                                                                       \
    M4_SUBSTEP(0, acur, brd, sac, sbc);                                     \
    M4_SUBSTEP(1, acur, brd, sac, sbc);                                     \
  } while (0)

  // steady state, two tiles per trip with every issue unconditional: the A
  // slots and the scale pairs are back where they were after two phases,
  // the three B slots have moved on by two
  int t = 0;
  for (; t + 3 < nt; t += 2) {
    M4_PHASE(t, aw0, aw1, bw0, bw2, sa0, sb0, sa1, sb1, true, true);
    M4_PHASE(t + 1, aw1, aw0, bw1, bw0, sa1, sb1, sa0, sb0, true, true);
    char* b0 = bw0; bw0 = bw2; bw2 = bw1; bw1 = b0;
  }
  // the last one to three tiles (t is even), issues guarded
  M4_PHASE(t, aw0, aw1, bw0, bw2, sa0, sb0, sa1, sb1, t + 1 < nt, t + 2 < nt);
  if (t + 1 < nt)
    M4_PHASE(t + 1, aw1, aw0, bw1, bw0, sa1, sb1, sa0, sb0, t + 2 < nt,
             false);
  if (t + 2 < nt)
    M4_PHASE(t + 2, aw0, aw1, bw2, bw1, sa0, sb0, sa1, sb1, false, false);
#undef M4_PHASE
#undef M4_SCALES_LANDED
#undef M4_LOAD_SCALES
#undef M4_SUBSTEP
#undef M4_MFMA
#undef M4_MFMA1
#undef M4_READ

  // N % 256 == 0: every wave's stripe is whole (WHOLE_STRIPES)
  tile_epilogue<EPI, HAS_BIAS, OUT_FP32, false, LIVE, true>(
      acc, bias, w3, nullptr, nullptr, C, M, N, m0, n0, wm, wn, fl, kg,
      live_rows);
}

// ---- host wrappers ---------------------------------------------------------

// what the scale layout asks of an [R, K] operand
static void m4_check_shape(const char* op, long long R, long long K) {
  TORCH_CHECK(R % 64 == 0 && K % M4_BK == 0, op,
              " requires rows%64==0 and K%256==0 (got ", R, "x", K, ")");
}

static void m4_check_out(const char* op, const at::Tensor& like,
                         const at::Tensor& q, const at::Tensor& s,
                         long long R, long long K) {
  TORCH_CHECK(q.is_cuda() && s.is_cuda() && q.device() == like.device() &&
                  s.device() == like.device() &&
                  q.scalar_type() == at::kByte &&
                  s.scalar_type() == at::kByte && q.is_contiguous() &&
                  s.is_contiguous(),
              op, ": q and s must be contiguous uint8 tensors on the "
              "input's device");
  TORCH_CHECK(q.numel() == R * K / 2 && s.numel() == R * K / 32, op,
              ": q must hold R*K/2 bytes and s R*K/32");
  TORCH_CHECK((uintptr_t)q.data_ptr() % 16 == 0 &&
                  (uintptr_t)s.data_ptr() % 8 == 0,
              op, ": q must be 16-byte and s 8-byte aligned");
}

// x [R, K] (fp32 or bf16) -> q [R, K/2], s [R*K/32], written in place
void quantize_mxfp4_hip(const at::Tensor& x, at::Tensor q, at::Tensor s) {
  const char* op = "quantize_mxfp4";
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2, op,
              ": x must be a contiguous 2-d cuda tensor");
  const long long R = x.size(0), K = x.size(1);
  m4_check_shape(op, R, K);
  m4_check_out(op, x, q, s, R, K);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0, op,
              ": x must be 16-byte aligned");
  const int k8 = (int)(K / 8);
  launch_quantiser(op, x, R * k8, [&](auto* xp, int blocks) {
    hipLaunchKernelGGL(quantize_mxfp4_kernel<std::decay_t<decltype(*xp)>>,
                       dim3(blocks), dim3(256), 0,
                       at::cuda::getCurrentCUDAStream(), xp,
                       q.data_ptr<unsigned char>(),
                       s.data_ptr<unsigned char>(), R, k8);
  });
}

// n_dev: only the first n_dev rows are computed; the rest of both outputs
// is left unwritten.
std::tuple<at::Tensor, at::Tensor> expand1d_mxfp4_hip(
    const at::Tensor& x, const at::Tensor& w,
    const c10::optional<at::Tensor>& b,
    const c10::optional<at::Tensor>& n_dev) {
  const char* op = "expand1d_mxfp4";
  const Expand1dArgs a = expand1d_args(op, x, w, b);
  TORCH_CHECK(x.is_contiguous() && w.is_cuda() && w.is_contiguous(), op,
              ": x and w must be contiguous cuda tensors");
  m4_check_shape(op, a.n, a.H);
  const int64_t* n_live = n_live_ptr(n_dev, x, op);
  auto q = at::empty({a.n, a.H / 2}, w.options().dtype(at::kByte));
  auto s = at::empty({a.n * a.H / 32}, w.options().dtype(at::kByte));
  if (a.grid == 0) return {q, s};
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_E1D_MXFP4(B_)                                                \
  hipLaunchKernelGGL((expand1d_mxfp4_kernel<B_>), dim3(a.grid), dim3(256),  \
                     0, stream, a.x, a.w, a.b, q.data_ptr<unsigned char>(), \
                     s.data_ptr<unsigned char>(), a.n, a.h8, n_live)
  if (a.b) LAUNCH_E1D_MXFP4(true);
  else     LAUNCH_E1D_MXFP4(false);
#undef LAUNCH_E1D_MXFP4
  return {q, s};
}

// The operands every MXFP4 GEMM op takes: codes aq [M, K/2], bq [N, K/2]
// (gemm_host.h's check) and their scale tensors.  `op` prefixes the error
// texts.
static MxGemm m4_gemm_operands(const char* op, const at::Tensor& aq,
                               const at::Tensor& as, const at::Tensor& bq,
                               const at::Tensor& bs) {
  // k_max: the per-lane staging offset is a 32-bit int
  static const GemmFormat fp4{torch::kUInt8, "fp4 code byte", 1, 2, M4_BK,
                              1ll << 24};
  MxGemm g(gemm256_operands(op, fp4, aq, bq));
  // the kernel's last phase runs whatever nt is
  TORCH_CHECK(g.K > 0, op, ": K must be positive");
  for (const at::Tensor* t : {&as, &bs})
    TORCH_CHECK(t->is_cuda() && t->device() == aq.device() &&
                    t->scalar_type() == torch::kUInt8 && t->is_contiguous(),
                op, ": scales must be contiguous uint8 cuda tensors on the "
                "codes' device");
  TORCH_CHECK(as.numel() == g.M * g.K / 32 && bs.numel() == g.N * g.K / 32,
              op, ": a scale tensor holds rows*K/32 bytes");
  TORCH_CHECK((uintptr_t)as.data_ptr() % 8 == 0 &&
                  (uintptr_t)bs.data_ptr() % 8 == 0,
              op, ": scales must be 8-byte aligned");
  g.sa_blk = as.data_ptr<unsigned char>();
  g.sb_blk = bs.data_ptr<unsigned char>();
  return g;
}

template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool LIVE = false>
static void m4_launch(const MxGemm& g) {
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((gemm_mxfp4_nt_kernel<EPI, HAS_BIAS, OUT_FP32, LIVE>),
                     g.grid(), dim3(M4_THREADS), 0, stream, g.a8(),
                     g.sa_blk, g.b8(), g.sb_blk, g.bias, g.w3, g.c, g.M, g.N,
                     g.K, g.n_live);
}

// C[M,N] = A[M,K] . B[N,K]^T over MXFP4 operands, optional fused bias+relu
// epilogue, fp32 or bf16 output.
at::Tensor gemm_mxfp4_nt_hip(const at::Tensor& aq, const at::Tensor& as,
                             const at::Tensor& bq, const at::Tensor& bs,
                             const c10::optional<at::Tensor>& bias, bool relu,
                             bool out_fp32) {
  const char* op = "gemm_mxfp4_nt";
  MxGemm g = m4_gemm_operands(op, aq, as, bq, bs);
  g.bias = epi_vec_n(op, "bias", bias, g.N);
  TORCH_CHECK(relu || !g.bias, op, ": bias requires the relu epilogue");
  auto opts = aq.options().dtype(out_fp32 ? torch::kFloat : torch::kBFloat16);
  auto C = torch::empty({g.M, g.N}, opts);
  if (g.empty()) return C;
  g.c = C.data_ptr();
  dispatch_epilogue(relu, g.bias != nullptr, out_fp32,
                    [&](auto e, auto hb, auto of) {
                      m4_launch<decltype(e)::value, decltype(hb)::value,
                                decltype(of)::value>(g);
                    });
  return C;
}

// y[M] = sum_col relu(A.B^T + b2) * w3 — the fp4 scoring forward's h2 GEMM
// and rowdot head in ONE kernel.  Caller adds the scalar b3.  With n_dev the
// row tiles past that live count return at once and y[n_dev:] stays 0.
at::Tensor gemm_mxfp4_relu_dot_hip(const at::Tensor& aq, const at::Tensor& as,
                                   const at::Tensor& bq, const at::Tensor& bs,
                                   const at::Tensor& b2, const at::Tensor& w3,
                                   const c10::optional<at::Tensor>& n_dev) {
  const char* op = "gemm_mxfp4_relu_dot";
  MxGemm g = m4_gemm_operands(op, aq, as, bq, bs);
  g.bias = epi_vec_n(op, "b2", b2, g.N);
  g.w3 = epi_vec_n(op, "w3", w3, g.N);
  TORCH_CHECK(g.bias && g.w3, op, ": b2 and w3 are required");
  g.n_live = n_live_ptr(n_dev, aq, op);
  auto y = torch::zeros({g.M}, aq.options().dtype(torch::kFloat));
  if (g.empty()) return y;
  g.c = y.data_ptr();
  if (g.n_live) m4_launch<Epi::ReluDot, true, true, true>(g);
  else          m4_launch<Epi::ReluDot, true, true>(g);
  return y;
}
