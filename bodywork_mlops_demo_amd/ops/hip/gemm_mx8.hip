// MX-FP8 (e4m3 / e5m2) 256x256-tile NT GEMM for gfx950 — the 2x-rate
// low-precision path.  ONE schedule: gemm_mx8_nt_1p_kernel, a single
// phase and a single barrier per K-tile.
//
// Why this shape: the non-scaled fp8 MFMAs (mfma_f32_16x16x32_fp8_fp8)
// run at the BF16 rate on CDNA4 — the ONLY 2x-rate fp8 instruction is
// the block-scaled __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4
// (K=128, per-32-element E8M0 scales, HW-fused dequant).  This kernel
// feeds it PER-TENSOR power-of-two scales: every lane passes the same
// E8M0 byte (the tensor's shared exponent), so the hardware dequant does
// the rescale for free and there is ZERO scale memory traffic in the
// K-loop.
//
// Geometry: 16 waves (4x4) per 1024-thread block, 64x64 of C per wave =
// 4x4 fragments.  BK = 128 fp8 bytes/row == gemm8.hip's BK=64 bf16
// (128 B/row), so a half-tile is the same 16 KiB and is staged the same
// way: ONE wave-level global_load_lds per wave per half-tile, the XOR
// swizzle carried on the glds SOURCE address.  One K-tile is ONE K=128
// MFMA per output fragment (vs four K=32 bf16 MFMAs); each lane's A/B
// fragment is 32 consecutive k bytes (two adjacent ds_read_b128).
//
// Schedule: A is double-buffered, B TRIPLE-buffered (LDS = 2x32 + 3x32 =
// 160 KB, the full CU), which is what lets one barrier per K-tile keep
// every overwrite barrier-separated.  Per tile T (slots: A T%2, B T%3):
//
//   wait vmcnt(2) [vmcnt(0) on the last tile]; barrier
//   issue A(T+1) -> slot (T+1)%2   [overwrites A(T-1), read last phase]
//   issue B(T+2) -> slot (T+2)%3   [overwrites B(T-1), read last phase]
//   read B(T) x4 frags + A mfrag 0,1; 8 MFMAs; read A mfrag 2,3; 8 MFMAs
//
// Landing proof: per phase the issue order is [A(T+1), B(T+2)], so at
// wait(T) the 2 newest outstanding glds are B(T+1)'s halves (issued at
// phase T-1 after A(T)) — vmcnt(2) proves A(T) and everything older
// (incl. B(T), issued at phase T-2) landed.  Near the end the guarded
// issues only SHRINK the outstanding set, and the final tile waits
// vmcnt(0).  Slot safety: both overwrites target buffers whose reads
// were consumed by the PREVIOUS phase's MFMAs, before this phase's
// barrier.
//
// History: the first version was a 2-phase port of gemm8.hip's schedule
// (two barriers per K-tile, 128 KB LDS) with optional supertile / XCD
// block remaps.  This schedule beat it by 6-10% on every shape at
// identical MFMA work (−20% wave cycles, profiles/r02_mx8_1p.md) and the
// remaps stayed within noise of the natural dispatch order
// (profiles/r02_mx8_pmc.md), so both were removed; they are in the
// history at commit 850e461.
//
// Numerics: A and B are e4m3 with per-tensor shared exponents ea, eb
// (value = 2^e * stored).  Scale operands sa = ea+127, sb = eb+127
// (E8M0); C = 2^(ea+eb) * (Aq . Bq) accumulated in fp32 by the MFMA.
// Power-of-two scaling keeps dequantisation exact.
//
// Training backward (gemm_mx8_nt_fmt): either operand may be e5m2 (the
// gradient format — the MFMA's cbsz/blgp immediates select it, both
// formats are one byte so the memory system is unchanged), either
// exponent may carry a per-step part read from device memory before the
// K-loop (so a captured step graph follows the gradient scale), and the
// Epi::MaskMul epilogue applies a 1-bit ReLU mask (dz1 = ... * m1).
//
// The reference computes its scoring forward in fp64 sklearn
// (stage_2_serve_model.py:78); this kernel is the opt-in low-precision
// serving/training path with MAPE parity gates in the tests.
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "bf16_utils.h"
#include "expand1d.h"
#include "host_checks.h"
#include "mfma_tile.h"

#define MX_BM 256
#define MX_BN 256
#define MX_BK 128           // fp8 elements per K-tile (128 bytes/row)
#define MX_THREADS 1024
#define MX_HTB (128 * 128)  // bytes per half-tile slot

typedef __attribute__((ext_vector_type(8))) int mx_i32x8;
typedef __attribute__((ext_vector_type(4))) int mx_i32x4;

// operand formats = the scaled MFMA's cbsz (A) / blgp (B) immediates
#define MX_FMT_E4M3 0
#define MX_FMT_E5M2 1

// DEV_SCALE: sa/sb arrive as (host exponent + 127), NOT range-checked;
// add the int32 unbiased exponent behind each non-null pointer and clamp
// to the E8M0 range.  One uniform load per operand, before the K-loop.
template <bool DEV_SCALE>
__device__ __forceinline__ void mx_dev_scales(int& sa, int& sb,
                                              const int* __restrict__ ea_dev,
                                              const int* __restrict__ eb_dev) {
  if (DEV_SCALE) {
    if (ea_dev) sa += *ea_dev;
    if (eb_dev) sb += *eb_dev;
    sa = min(max(sa, 0), 254);
    sb = min(max(sb, 0), 254);
  }
}

// stage one [128 rows][128 B] half-tile: 1024 16-B chunks, 1024 threads
// -> ONE wave-level glds per wave (identical to gemm8's g8_stage_half).
__device__ __forceinline__ void mx_stage_half(char* __restrict__ slot,
                                              const char* __restrict__ base,
                                              int off0) {
  const int wave = threadIdx.x >> 6;
  glds16(base + off0, slot + wave * 1024);
}

// ---- per-tensor e4m3 quantisation ----------------------------------------
//
// x (bf16 or fp32) -> e4m3 bytes, value = 2^e * stored.  e is chosen
// host-side so |x|max / 2^e <= 448 (no saturation).  The HW fast-path
// packed convert (cvt_pk_fp8_f32) rounds to nearest-even.
template <typename T>
__global__ void quantize_e4m3_kernel(const T* __restrict__ x,
                                     unsigned char* __restrict__ out,
                                     long long n, float inv_scale) {
  long long i = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i * 2 + 1 < n; i += stride) {
    float v0, v1;
    if constexpr (sizeof(T) == 2) {
      v0 = bf16_to_f32(((const bf16_t*)x)[i * 2]);
      v1 = bf16_to_f32(((const bf16_t*)x)[i * 2 + 1]);
    } else {
      v0 = ((const float*)x)[i * 2];
      v1 = ((const float*)x)[i * 2 + 1];
    }
    // packed RNE convert; lower 16 bits hold the two e4m3 bytes
    int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v0 * inv_scale,
                                                 v1 * inv_scale, 0, false);
    *(unsigned short*)(out + i * 2) = (unsigned short)(packed & 0xFFFF);
  }
  // odd tail element (single-element convert via the same packed op)
  if (i * 2 < n && n % 2 == 1 && i * 2 == n - 1) {
    float v = sizeof(T) == 2 ? bf16_to_f32(((const bf16_t*)x)[n - 1])
                             : ((const float*)x)[n - 1];
    int packed =
        __builtin_amdgcn_cvt_pk_fp8_f32(v * inv_scale, 0.0f, 0, false);
    out[n - 1] = (unsigned char)(packed & 0xFF);
  }
}

// ---- the MX GEMM kernel: one phase, one barrier per K-tile -----------------
//
// Schedule and landing proof: see the file header.
#define P1_ASLOT(buf, half) (lds + ((buf) * 2 + (half)) * MX_HTB)
#define P1_BSLOT(buf, half) (lds + (4 + (buf) * 2 + (half)) * MX_HTB)
#define MX_KOFF(T) ((long long)(T) * MX_BK)  // byte offset of K-tile T in a row

template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool EMIT_MASK = false,
          int AFMT = MX_FMT_E4M3, int BFMT = MX_FMT_E4M3,
          bool DEV_SCALE = false, bool LIVE = false>
__launch_bounds__(MX_THREADS)
__global__ void gemm_mx8_nt_1p_kernel(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ B,
    const float* __restrict__ bias, const float* __restrict__ w3,
    unsigned char* __restrict__ mask_out, void* __restrict__ C, long long M,
    long long N, long long K, int sa, int sb,
    const int* __restrict__ ea_dev = nullptr,  // DEV_SCALE only
    const int* __restrict__ eb_dev = nullptr,
    const unsigned char* __restrict__ mask_in = nullptr,  // MASK_MUL only
    const int64_t* __restrict__ n_live = nullptr) {       // LIVE only
  __shared__ char lds[10 * MX_HTB];  // A 2 slots + B 3 slots, 160 KB
  mx_dev_scales<DEV_SCALE>(sa, sb, ea_dev, eb_dev);
  const long long m0 = (long long)blockIdx.y * MX_BM;
  int live_rows = MX_BM;
  if constexpr (LIVE) {
    static_assert(EPI == Epi::ReluDot, "live rows: scoring head only");
    if (!tile_live_rows<MX_BM>(n_live, M, m0, live_rows)) return;
  }
  const long long n0 = (long long)blockIdx.x * MX_BN;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 2;
  const int wn = wave & 3;
  const int fl = lane & 15;
  const int kg = lane >> 4;
  // XOR swizzle at 32-BYTE granularity — the fp8 fragment size, so a
  // fragment is two ADJACENT b128 reads (chunk32 c of row r lives at
  // (c ^ (r & 3)) * 32).  Measured equivalent to the 16-B-chunk
  // stride-2 variant: SQ_LDS_BANK_CONFLICT reads exactly 4 events per
  // v_mfma_scale under BOTH layouts (6.711e8 = 4x the MFMA count,
  // unchanged by the swizzle change) — an artifact of the scaled-MFMA
  // instruction, not real ds_read serialisation
  // (profiles/r02_mx8_pmc.md).
  const int swz = fl & 3;
  const int nt = (int)(K / MX_BK);
  const int a_inhalf = (wm & 1) * 64;
  const int b_inhalf = (wn & 1) * 64;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // slot indices only affect LDS ADDRESSES (never register-array
  // indices), so the A slots swap and the B slots rotate as plain
  // pointer variables — the loop body is ONE phase, which keeps
  // register pressure low (a 6-tile compile-time unroll of this
  // schedule spilled ~400 VGPRs)
  char* aw_cur = P1_ASLOT(0, 0);
  char* aw_nxt = P1_ASLOT(1, 0);
  char* bw0 = P1_BSLOT(0, 0);  // holds B(T)
  char* bw1 = P1_BSLOT(1, 0);  // holds B(T+1) (in flight or staged)
  char* bw2 = P1_BSLOT(2, 0);  // staging target for B(T+2)
  // this wave reads its half directly: precompute read bases
#define P1_AR_BASE(slotp) ((slotp) + (wm >> 1) * MX_HTB)
#define P1_BR_BASE(slotp) ((slotp) + (wn >> 1) * MX_HTB)

  // one fragment = 32 consecutive k bytes = LDS chunks {2kg, 2kg+1}
  // (XOR-swizzled), read as two b128s straight into the halves of the
  // i32x8 MFMA operand (a per-element insertelement assembly costs ~5
  // v_mov per fragment — 304 v_movs per unrolled loop, measured in the
  // .s — so the loads are written through the operand's i32x4 halves
  // to land in its own register quadruples)
#define P1_READ8(dst, rowbase, rowoff)                                      \
  do {                                                                      \
    const char* _rb = (rowbase) + (rowoff) * 128 + ((kg ^ swz) * 32);       \
    ((mx_i32x4*)&(dst))[0] = *(const mx_i32x4*)(_rb);                       \
    ((mx_i32x4*)&(dst))[1] = *(const mx_i32x4*)(_rb + 16);                  \
  } while (0)

  mx_i32x8 a_q[2];
  mx_i32x8 b_t[4];

  // per-lane staging byte offset (tile-invariant): thread ci stages the
  // 16-B half `ci&1` of 32-B chunk `(ci&7)>>1` of row `ci>>3`; the
  // 32-B chunk lands at (chunk ^ (row & 3)) * 32 in LDS, halves stay
  // adjacent, so the glds SOURCE address carries the swizzle exactly as
  // in the bf16 kernel
  int stg_off;
  {
    int ci = (int)threadIdx.x;
    int row = ci >> 3;
    int c32 = ((ci & 7) >> 1) ^ (row & 3);
    stg_off = (int)(row * K + (c32 * 32 + (ci & 1) * 16));
  }
  const char* Ah0 = (const char*)(A + m0 * K);
  const char* Ah1 = (const char*)(A + (m0 + 128) * K);
  const char* Bh0 = (const char*)(B + n0 * K);
  const char* Bh1 = (const char*)(B + (n0 + 128) * K);

  // prologue: A(0), B(0), B(1)
  mx_stage_half(aw_cur, Ah0, stg_off);
  mx_stage_half(aw_cur + MX_HTB, Ah1, stg_off);
  mx_stage_half(bw0, Bh0, stg_off);
  mx_stage_half(bw0 + MX_HTB, Bh1, stg_off);
  if (nt > 1) {
    mx_stage_half(bw1, Bh0 + MX_KOFF(1), stg_off);
    mx_stage_half(bw1 + MX_HTB, Bh1 + MX_KOFF(1), stg_off);
  }

#define P1_MFMA(acc_i, afrag)                                               \
  _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                          \
      acc[acc_i][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(    \
          afrag, b_t[nf], acc[acc_i][nf], AFMT, BFMT, 0, sa, 0, sb)

  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt)
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 < nt) {
      mx_stage_half(aw_nxt, Ah0 + MX_KOFF(t + 1), stg_off);
      mx_stage_half(aw_nxt + MX_HTB, Ah1 + MX_KOFF(t + 1), stg_off);
    }
    if (t + 2 < nt) {
      mx_stage_half(bw2, Bh0 + MX_KOFF(t + 2), stg_off);
      mx_stage_half(bw2 + MX_HTB, Bh1 + MX_KOFF(t + 2), stg_off);
    }
    {
      const char* br = P1_BR_BASE(bw0);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        P1_READ8(b_t[nf], br, b_inhalf + nf * 16 + fl);
    }
    {
      const char* ar = P1_AR_BASE(aw_cur);
      P1_READ8(a_q[0], ar, a_inhalf + 0 * 16 + fl);
      P1_READ8(a_q[1], ar, a_inhalf + 1 * 16 + fl);
      __builtin_amdgcn_s_setprio(1);
      P1_MFMA(0, a_q[0]);
      P1_MFMA(1, a_q[1]);
      __builtin_amdgcn_s_setprio(0);
      P1_READ8(a_q[0], ar, a_inhalf + 2 * 16 + fl);
      P1_READ8(a_q[1], ar, a_inhalf + 3 * 16 + fl);
      __builtin_amdgcn_s_setprio(1);
      P1_MFMA(2, a_q[0]);
      P1_MFMA(3, a_q[1]);
      __builtin_amdgcn_s_setprio(0);
    }
    // rotate slots: A swaps, B rotates forward
    char* tmp = aw_cur; aw_cur = aw_nxt; aw_nxt = tmp;
    char* b0 = bw0; bw0 = bw1; bw1 = bw2; bw2 = b0;
  }
#undef P1_MFMA
#undef P1_READ8
#undef P1_AR_BASE
#undef P1_BR_BASE

  // N % 256 == 0: every wave's mask stripe is whole (WHOLE_STRIPES)
  tile_epilogue<EPI, HAS_BIAS, OUT_FP32, EMIT_MASK, LIVE, true>(
      acc, bias, w3, mask_in, mask_out, C, M, N, m0, n0, wm, wn, fl, kg,
      live_rows);
}

// ---- fused rank-1 expand -> e4m3 ------------------------------------------
//
// The MLP fp8 scoring forward's layer 1: h1 = relu(x*w + b) emitted
// DIRECTLY as e4m3 bytes (value = 2^e * stored).  Unfused, the path
// writes h1 as bf16 (2 B/elem), re-reads it (2 B) and writes the fp8
// copy (1 B) — 5 bytes of HBM per element; this kernel writes 1.
template <bool HAS_BIAS>
__global__ void expand1d_e4m3_kernel(const float* __restrict__ x,
                                     const bf16_t* __restrict__ w,
                                     const bf16_t* __restrict__ b,
                                     unsigned char* __restrict__ out,
                                     long long n, int h8 /* H/8 */,
                                     float inv_scale,
                                     const int64_t* __restrict__ n_live) {
  // n_live, when given, is the live row count (device int64[1], clamped to
  // [0, n]): rows at or past it are neither read nor written
  if (n_live != nullptr) n = live_count(n_live, n);
  e1d_for_each_chunk(n, h8, [&](long long row, int c8) {
    float acc[8];
    e1d_axpb<true, HAS_BIAS>(x[row], w, b, c8, acc);
    e1d_store_e4m3(out, e1d_offset(row, h8, c8), acc, inv_scale);
  });
}

// ---- dual-emit rank-1 expand: bf16 + 1-bit mask + e4m3 --------------------
//
// The MLP fp8 TRAINING forward's layer 1: h1 = relu(x*w + b) is needed
// as bf16 (dW2 = h1^T . dz2 in the backward), as its 1-bit mask (masked
// backward) and as e4m3 (A operand of the MX GEMM).  One pass writes all
// three from the same fp32 value (3.125 B/element) instead of a separate
// quantise pass re-reading the bf16 copy (+3 B/element).  Arithmetic is
// that of expand1d_kernel<relu, emit_mask> and expand1d_e4m3_kernel, so
// each output is bit-identical to the single-output kernel's.
template <bool HAS_BIAS>
__global__ void expand1d_bf16_e4m3_kernel(
    const float* __restrict__ x, const bf16_t* __restrict__ w,
    const bf16_t* __restrict__ b, bf16_t* __restrict__ out,
    unsigned char* __restrict__ mask_out, unsigned char* __restrict__ out8,
    long long n, int h8 /* H/8 */, float inv_scale) {
  e1d_for_each_chunk(n, h8, [&](long long row, int c8) {
    float acc[8];
    e1d_axpb<true, HAS_BIAS>(x[row], w, b, c8, acc);
    const long long o = e1d_offset(row, h8, c8);
    mask_out[row * h8 + c8] = e1d_mask_bits(acc);
    e1d_store_bf16(out, o, acc);
    e1d_store_e4m3(out8, o, acc, inv_scale);
  });
}

// ---- e5m2 (gradient format) support kernels -------------------------------
//
// mx_e5m2_prescale and mx_cvt2_e5m2 (the defined-saturation RNE convert) are
// in expand1d.h.

// Per-step gradient exponent, computed on the device so a captured step
// never syncs: a = max|x| * max|w| (fp32) bounds every |x[i]*w[j]|
// because fp32 multiplication is monotone; out[0] = smallest e with
// a / 2^e <= 57344, clamped to [-127,127]; 0 when a is 0 or non-finite.
// The maxima are taken over the |value| BIT PATTERNS (monotone as
// unsigned ints, NaN/inf sort above every finite value), so a NaN input
// reaches the final test instead of being dropped by fmaxf.  The
// exponent comes from the float's fields (a = 1.f * 2^(E-127), and
// 57344 = 1.75 * 2^15), so the boundary is exact.  ONE block, no
// atomics, order-independent integer max -> bitwise deterministic.
__launch_bounds__(1024)
__global__ void amax_exponent_e5m2_kernel(const float* __restrict__ x,
                                          long long n,
                                          const bf16_t* __restrict__ w,
                                          long long H,
                                          int* __restrict__ out) {
  __shared__ unsigned int red[2][16];
  const int tid = (int)threadIdx.x;
  unsigned int mx = 0u, mw = 0u;
  for (long long i = tid; i < n; i += 1024)
    mx = max(mx, __float_as_uint(x[i]) & 0x7FFFFFFFu);
  for (long long i = tid; i < H; i += 1024)
    mw = max(mw, __float_as_uint(bf16_to_f32(w[i])) & 0x7FFFFFFFu);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = max(mx, (unsigned int)__shfl_xor((int)mx, off, 64));
    mw = max(mw, (unsigned int)__shfl_xor((int)mw, off, 64));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = mx;
    red[1][tid >> 6] = mw;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < 16; ++k) {
      mx = max(mx, red[0][k]);
      mw = max(mw, red[1][k]);
    }
    const float a = __uint_as_float(mx) * __uint_as_float(mw);
    const unsigned int bits = __float_as_uint(a) & 0x7FFFFFFFu;
    const int E = (int)(bits >> 23);
    const unsigned int man = bits & 0x7FFFFFu;
    int e;
    if (bits == 0u || E == 255)
      e = 0;  // zero, inf or nan
    else if (E == 0)
      e = -127;  // subnormal product: far below the clamp
    else
      e = E - 127 - (man <= 0x600000u ? 15 : 14);
    out[0] = min(max(e, -127), 127);
  }
}

// x (bf16 or fp32) -> e5m2 bytes, value = 2^e * stored; e = e_host +
// (*e_dev if given).
template <typename T>
__global__ void quantize_e5m2_kernel(const T* __restrict__ x,
                                     unsigned char* __restrict__ out,
                                     long long n, int e_host,
                                     const int* __restrict__ e_dev) {
  const int e = e_host + (e_dev ? *e_dev : 0);
  long long i = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long pairs = (n + 1) / 2;
  for (; i < pairs; i += stride) {
    const bool has1 = i * 2 + 1 < n;
    float v0, v1 = 0.0f;
    if constexpr (sizeof(T) == 2) {
      v0 = bf16_to_f32(((const bf16_t*)x)[i * 2]);
      if (has1) v1 = bf16_to_f32(((const bf16_t*)x)[i * 2 + 1]);
    } else {
      v0 = ((const float*)x)[i * 2];
      if (has1) v1 = ((const float*)x)[i * 2 + 1];
    }
    unsigned int pk =
        mx_cvt2_e5m2(mx_e5m2_prescale(v0, e), mx_e5m2_prescale(v1, e));
    if (has1)
      *(unsigned short*)(out + i * 2) = (unsigned short)pk;
    else
      out[i * 2] = (unsigned char)(pk & 0xFFu);  // odd tail element
  }
}

// Dual-emit masked rank-1 expand for the backward: dz2 = outer(x, w) *
// bit(mask) as bf16 (bit-identical to expand1d_kernel<false, false, true,
// false>; colsum for db2 reads it) AND as e5m2 bytes of the bf16-ROUNDED
// value with the exponent read from e_dev (so it equals
// quantize_e5m2(bf16 output, e_dev)).
__global__ void expand1d_bf16_e5m2_kernel(
    const float* __restrict__ x, const bf16_t* __restrict__ w,
    const unsigned char* __restrict__ mask, const int* __restrict__ e_dev,
    bf16_t* __restrict__ out, unsigned char* __restrict__ out8, long long n,
    int h8 /* H/8 */) {
  const int e = *e_dev;
  e1d_for_each_chunk(n, h8, [&](long long row, int c8) {
    float acc[8], rb[8];
    e1d_axpb<false, false>(x[row], w, nullptr, c8, acc);
    e1d_apply_mask(mask[row * h8 + c8], acc);
    const long long o = e1d_offset(row, h8, c8);
    bf16x8_to_f32(e1d_store_bf16(out, o, acc), rb);
    e1d_store_e5m2(out8, o, rb, e);
  });
}

// Byte transpose dst[C,R] = src[R,C]^T for the wgrad operands (both must
// be K-contiguous over the batch).  128(src rows) x 64(src cols) LDS
// tile, 16-B global loads and stores; R % 16 == 0 and C % 16 == 0 (host
// checked) make every 16-B chunk wholly inside or wholly outside, edge
// tiles are guarded per chunk.  LDS rows are 17 dwords (68 B): the
// column-gather of the write phase reads rows 16 apart, which the odd
// dword stride spreads over distinct banks.
#define TU8_TR 128
#define TU8_TC 64
__launch_bounds__(256)
__global__ void transpose_u8_kernel(const unsigned char* __restrict__ src,
                                    unsigned char* __restrict__ dst,
                                    long long R, long long C) {
  __shared__ unsigned int tile[TU8_TR][17];
  const long long r0 = (long long)blockIdx.y * TU8_TR;
  const long long c0 = (long long)blockIdx.x * TU8_TC;
  const int tid = (int)threadIdx.x;
  // load: 128 rows x 4 chunks = 512 chunks, 2 passes
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int ch = tid & 3;
    const int tr = (tid >> 2) + p * 64;
    const long long r = r0 + tr;
    const long long c = c0 + ch * 16;
    if (r < R && c < C) {
      const mx_i32x4 v = *(const mx_i32x4*)(src + r * C + c);
      tile[tr][ch * 4 + 0] = (unsigned int)v[0];
      tile[tr][ch * 4 + 1] = (unsigned int)v[1];
      tile[tr][ch * 4 + 2] = (unsigned int)v[2];
      tile[tr][ch * 4 + 3] = (unsigned int)v[3];
    }
  }
  __syncthreads();
  // store: out row = src col (64), out chunk = 16 src rows (8 chunks);
  // pass p handles chunks 4p..4p+3 so a wave's four chunks sit 16 LDS
  // rows apart (distinct banks) and 4 lanes fill 64 contiguous bytes
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int tc = (tid & 3) + p * 4;
    const int oc = tid >> 2;
    const long long orow = c0 + oc;
    const long long ocol = r0 + tc * 16;
    if (orow < C && ocol < R) {
      const unsigned char* tb = (const unsigned char*)&tile[0][0];
      mx_i32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned int wq = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          wq |= (unsigned int)tb[(tc * 16 + q * 4 + k) * 68 + oc] << (8 * k);
        v[q] = (int)wq;
      }
      *(mx_i32x4*)(dst + orow * R + ocol) = v;
    }
  }
}

// ---- host wrappers --------------------------------------------------------

// n_dev: only the first n_dev rows are computed; the rest of the output
// is left unwritten.
at::Tensor expand1d_e4m3_hip(const at::Tensor& x, const at::Tensor& w,
                             const c10::optional<at::Tensor>& b, int64_t e,
                             const c10::optional<at::Tensor>& n_dev) {
  const Expand1dArgs a = expand1d_args("expand1d_e4m3", x, w, b);
  const int64_t* n_live = n_live_ptr(n_dev, x, "expand1d_e4m3");
  auto out = at::empty({a.n, a.H}, w.options().dtype(at::kByte));
  if (a.grid == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  float inv_scale = ldexpf(1.0f, (int)-e);
#define LAUNCH_E1D_E4M3(B_)                                                 \
  hipLaunchKernelGGL((expand1d_e4m3_kernel<B_>), dim3(a.grid), dim3(256),   \
                     0, stream, a.x, a.w, a.b,                              \
                     out.data_ptr<unsigned char>(), a.n, a.h8, inv_scale,   \
                     n_live)
  if (a.b) LAUNCH_E1D_E4M3(true);
  else     LAUNCH_E1D_E4M3(false);
#undef LAUNCH_E1D_E4M3
  return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> expand1d_bf16_e4m3_hip(
    const at::Tensor& x, const at::Tensor& w,
    const c10::optional<at::Tensor>& b, int64_t e) {
  const Expand1dArgs a = expand1d_args("expand1d_bf16_e4m3", x, w, b);
  auto out = at::empty({a.n, a.H}, w.options());
  auto mask_out = at::empty({a.n, a.H / 8}, w.options().dtype(at::kByte));
  auto out8 = at::empty({a.n, a.H}, w.options().dtype(at::kByte));
  if (a.grid == 0) return {out, mask_out, out8};
  auto stream = at::cuda::getCurrentCUDAStream();
  float inv_scale = ldexpf(1.0f, (int)-e);
#define LAUNCH_E1D_BF16_E4M3(B_)                                            \
  hipLaunchKernelGGL((expand1d_bf16_e4m3_kernel<B_>), dim3(a.grid),         \
                     dim3(256), 0, stream, a.x, a.w, a.b,                   \
                     (bf16_t*)out.data_ptr(),                               \
                     mask_out.data_ptr<unsigned char>(),                    \
                     out8.data_ptr<unsigned char>(), a.n, a.h8, inv_scale)
  if (a.b) LAUNCH_E1D_BF16_E4M3(true);
  else     LAUNCH_E1D_BF16_E4M3(false);
#undef LAUNCH_E1D_BF16_E4M3
  return {out, mask_out, out8};
}

at::Tensor quantize_e4m3_hip(const at::Tensor& x, int64_t e) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "quantize_e4m3: cuda contig");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 ||
                  torch::kFloat == x.scalar_type(),
              "quantize_e4m3: bf16 or fp32 input");
  auto out = torch::empty_like(x, x.options().dtype(torch::kUInt8));
  long long n = x.numel();
  if (n == 0) return out;
  float inv_scale = ldexpf(1.0f, (int)-e);
  auto stream = at::cuda::getCurrentCUDAStream();
  long long pairs = (n + 1) / 2;
  int threads = 256;
  int blocks = (int)std::min<long long>((pairs + threads - 1) / threads,
                                        8192);
  if (x.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(quantize_e4m3_kernel<short>, dim3(blocks),
                       dim3(threads), 0, stream,
                       (const short*)x.data_ptr(),
                       out.data_ptr<unsigned char>(), n, inv_scale);
  else
    hipLaunchKernelGGL(quantize_e4m3_kernel<float>, dim3(blocks),
                       dim3(threads), 0, stream, x.data_ptr<float>(),
                       out.data_ptr<unsigned char>(), n, inv_scale);
  return out;
}

// ---- MX GEMM ops: one operand check, one launcher --------------------------

// Everything a gemm_mx8_nt_1p_kernel launch takes.  mx_gemm_operands
// fills the problem and the operand pointers; each op sets the scales and
// the epilogue pointers it uses and leaves the rest null.
struct MxGemm {
  long long M = 0, N = 0, K = 0;
  dim3 grid;
  const unsigned char* a = nullptr;
  const unsigned char* b = nullptr;
  int sa = 127, sb = 127;             // E8M0 bytes (host part)
  const int* ea_dev = nullptr;        // DEV_SCALE
  const int* eb_dev = nullptr;
  const float* bias = nullptr;        // BIAS_RELU / RELU_DOT
  const float* w3 = nullptr;          // RELU_DOT
  unsigned char* mask_out = nullptr;  // EMIT_MASK
  const unsigned char* mask_in = nullptr;  // MASK_MUL
  const int64_t* n_live = nullptr;         // LIVE
  void* c = nullptr;
  bool empty() const { return M == 0 || N == 0; }  // nothing to launch
};

// The operand pair every MX GEMM op takes: a8 [M,K] and b8 [N,K] fp8
// bytes.  `op` prefixes the error texts.
static MxGemm mx_gemm_operands(const char* op, const at::Tensor& a8,
                               const at::Tensor& b8) {
  TORCH_CHECK(a8.is_cuda() && b8.is_cuda(), op, ": cuda tensors");
  TORCH_CHECK(a8.scalar_type() == torch::kUInt8 &&
                  b8.scalar_type() == torch::kUInt8,
              op, ": fp8 byte tensors");
  TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.size(1) == b8.size(1),
              op, ": [M,K]x[N,K]");
  TORCH_CHECK(a8.is_contiguous() && b8.is_contiguous(), op,
              ": operands must be contiguous");
  MxGemm g;
  g.M = a8.size(0), g.K = a8.size(1), g.N = b8.size(0);
  TORCH_CHECK(g.M % MX_BM == 0 && g.N % MX_BN == 0 && g.K % MX_BK == 0, op,
              " requires M%256==0, N%256==0, K%128==0 (got ", g.M, "x", g.N,
              "x", g.K, ")");
  TORCH_CHECK((uintptr_t)a8.data_ptr() % 16 == 0 &&
                  (uintptr_t)b8.data_ptr() % 16 == 0,
              op, ": operands must be 16-byte aligned");
  g.grid = dim3((unsigned)(g.N / MX_BN), (unsigned)(g.M / MX_BM));
  g.a = a8.data_ptr<unsigned char>();
  g.b = b8.data_ptr<unsigned char>();
  return g;
}

// host exponent -> E8M0 byte; out-of-range stays loud
static int mx_e8m0(const char* op, int64_t e) {
  TORCH_CHECK(-127 <= e && e <= 127, op,
              ": per-tensor exponent out of E8M0 range");
  return (int)e + 127;
}

// optional fp32 [N] epilogue vector (bias, b2, w3) -> pointer, nullptr
// when absent
static const float* mx_vec_n(const char* op, const char* what,
                             const c10::optional<at::Tensor>& v,
                             long long N) {
  if (!v.has_value() || !v->defined()) return nullptr;
  TORCH_CHECK(v->is_cuda() && v->scalar_type() == torch::kFloat &&
                  v->numel() == N && v->is_contiguous(),
              op, ": ", what, " must be a contiguous fp32 [N] cuda tensor");
  return v->data_ptr<float>();
}

template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool EMIT_MASK = false,
          int AFMT = MX_FMT_E4M3, int BFMT = MX_FMT_E4M3,
          bool DEV_SCALE = false, bool LIVE = false>
static void mx_launch(const MxGemm& g) {
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((gemm_mx8_nt_1p_kernel<EPI, HAS_BIAS, OUT_FP32, EMIT_MASK,
                                            AFMT, BFMT, DEV_SCALE, LIVE>),
                     g.grid, dim3(MX_THREADS), 0, stream, g.a, g.b, g.bias,
                     g.w3, g.mask_out, g.c, g.M, g.N, g.K, g.sa, g.sb,
                     g.ea_dev, g.eb_dev, g.mask_in, g.n_live);
}

// C[M,N] = 2^(ea+eb) * (A[M,K]e4m3 . B[N,K]e4m3^T), optional fused
// bias+relu epilogue, fp32 or bf16 output.
at::Tensor gemm_mx8_nt_hip(const at::Tensor& a8, int64_t ea,
                           const at::Tensor& b8, int64_t eb,
                           const c10::optional<at::Tensor>& bias, bool relu,
                           bool out_fp32) {
  const char* op = "gemm_mx8_nt";
  MxGemm g = mx_gemm_operands(op, a8, b8);
  g.sa = mx_e8m0(op, ea);
  g.sb = mx_e8m0(op, eb);
  g.bias = mx_vec_n(op, "bias", bias, g.N);
  TORCH_CHECK(relu || !g.bias, op, ": bias requires relu epilogue for now");
  auto opts = a8.options().dtype(out_fp32 ? torch::kFloat : torch::kBFloat16);
  auto C = torch::empty({g.M, g.N}, opts);
  if (g.empty()) return C;
  g.c = C.data_ptr();
  if (!relu) {
    if (out_fp32) mx_launch<Epi::None, false, true>(g);
    else          mx_launch<Epi::None, false, false>(g);
  } else if (g.bias) {
    if (out_fp32) mx_launch<Epi::BiasRelu, true, true>(g);
    else          mx_launch<Epi::BiasRelu, true, false>(g);
  } else {
    if (out_fp32) mx_launch<Epi::BiasRelu, false, true>(g);
    else          mx_launch<Epi::BiasRelu, false, false>(g);
  }
  return C;
}

// y[M] = sum_col relu(a8.b8^T dequant + b2) * w3  — the MLP scoring
// forward's h2 GEMM and rowdot head in ONE kernel: the [M,N] activation
// tensor is never written to HBM.  Caller adds the scalar b3.  With n_dev
// the row tiles past that live count return at once and y[n_dev:] stays 0.
at::Tensor gemm_mx8_relu_dot_hip(const at::Tensor& a8, int64_t ea,
                                 const at::Tensor& b8, int64_t eb,
                                 const at::Tensor& b2, const at::Tensor& w3,
                                 const c10::optional<at::Tensor>& n_dev) {
  const char* op = "gemm_mx8_relu_dot";
  MxGemm g = mx_gemm_operands(op, a8, b8);
  g.sa = mx_e8m0(op, ea);
  g.sb = mx_e8m0(op, eb);
  g.bias = mx_vec_n(op, "b2", b2, g.N);
  g.w3 = mx_vec_n(op, "w3", w3, g.N);
  TORCH_CHECK(g.bias && g.w3, op, ": b2 and w3 are required");
  g.n_live = n_live_ptr(n_dev, a8, op);
  auto y = torch::zeros({g.M}, a8.options().dtype(torch::kFloat));
  if (g.empty()) return y;
  g.c = y.data_ptr();
  if (g.n_live)
    mx_launch<Epi::ReluDot, true, true, false, MX_FMT_E4M3, MX_FMT_E4M3,
              false, true>(g);
  else
    mx_launch<Epi::ReluDot, true, true>(g);
  return y;
}

// (h2, mask) = relu(a8.b8^T dequant + bias) as bf16 AND its 1-bit ReLU
// mask (uint8 [M, N/8]) in one pass — the MLP fp8 TRAINING forward's h2
// GEMM (the MX twin of linear_relu_mask_bf16).  h2 is bit-identical to
// gemm_mx8_nt(..., relu=true, out_fp32=false).
std::tuple<at::Tensor, at::Tensor> gemm_mx8_relu_mask_hip(
    const at::Tensor& a8, int64_t ea, const at::Tensor& b8, int64_t eb,
    const c10::optional<at::Tensor>& bias) {
  const char* op = "gemm_mx8_relu_mask";
  MxGemm g = mx_gemm_operands(op, a8, b8);
  g.sa = mx_e8m0(op, ea);
  g.sb = mx_e8m0(op, eb);
  g.bias = mx_vec_n(op, "bias", bias, g.N);
  auto C = torch::empty({g.M, g.N}, a8.options().dtype(torch::kBFloat16));
  auto mask = torch::empty({g.M, g.N / 8}, a8.options());
  if (g.empty()) return {C, mask};
  g.c = C.data_ptr();
  g.mask_out = mask.data_ptr<unsigned char>();
  if (g.bias) mx_launch<Epi::BiasRelu, true, false, true>(g);
  else        mx_launch<Epi::BiasRelu, false, false, true>(g);
  return {C, mask};
}

// ---- training-backward ops: e5m2 operands, device exponents, mask-mul -----

// optional int32[1] device exponent -> pointer (nullptr when absent)
static const int* mx_edev_ptr(const c10::optional<at::Tensor>& e,
                              const at::Tensor& like, const char* what) {
  if (!e.has_value() || !e->defined()) return nullptr;
  TORCH_CHECK(e->is_cuda() && e->device() == like.device() &&
                  e->scalar_type() == torch::kInt32 && e->numel() == 1,
              what, ": device exponent must be an int32[1] tensor on the "
              "operand's device");
  return e->data_ptr<int>();
}

at::Tensor amax_exponent_e5m2_hip(const at::Tensor& x, const at::Tensor& w) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat,
              "amax_exponent_e5m2: x must be contiguous fp32 cuda");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
                  w.scalar_type() == torch::kBFloat16,
              "amax_exponent_e5m2: w must be contiguous bf16 cuda");
  auto out = torch::empty({1}, x.options().dtype(torch::kInt32));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(amax_exponent_e5m2_kernel, dim3(1), dim3(1024), 0,
                     stream, x.data_ptr<float>(), (long long)x.numel(),
                     (const bf16_t*)w.data_ptr(), (long long)w.numel(),
                     out.data_ptr<int>());
  return out;
}

at::Tensor quantize_e5m2_hip(const at::Tensor& x, int64_t e,
                             const c10::optional<at::Tensor>& e_dev) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "quantize_e5m2: cuda contig");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 ||
                  x.scalar_type() == torch::kFloat,
              "quantize_e5m2: bf16 or fp32 input");
  TORCH_CHECK(-127 <= e && e <= 127, "quantize_e5m2: exponent out of range");
  const int* edp = mx_edev_ptr(e_dev, x, "quantize_e5m2");
  auto out = torch::empty_like(x, x.options().dtype(torch::kUInt8));
  long long n = x.numel();
  if (n == 0) return out;
  auto stream = at::cuda::getCurrentCUDAStream();
  long long pairs = (n + 1) / 2;
  int threads = 256;
  int blocks = (int)std::min<long long>((pairs + threads - 1) / threads,
                                        8192);
  if (x.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(quantize_e5m2_kernel<short>, dim3(blocks),
                       dim3(threads), 0, stream, (const short*)x.data_ptr(),
                       out.data_ptr<unsigned char>(), n, (int)e, edp);
  else
    hipLaunchKernelGGL(quantize_e5m2_kernel<float>, dim3(blocks),
                       dim3(threads), 0, stream, x.data_ptr<float>(),
                       out.data_ptr<unsigned char>(), n, (int)e, edp);
  return out;
}

std::tuple<at::Tensor, at::Tensor> expand1d_bf16_e5m2_hip(
    const at::Tensor& x, const at::Tensor& w, const at::Tensor& mask,
    const at::Tensor& e_dev) {
  const char* op = "expand1d_bf16_e5m2";
  const Expand1dArgs a = expand1d_args(op, x, w, c10::nullopt);
  TORCH_CHECK(x.is_contiguous() && w.is_cuda() && w.is_contiguous(), op,
              ": x and w must be contiguous cuda tensors");
  TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() &&
                  mask.scalar_type() == at::kByte &&
                  mask.numel() == a.n * a.h8,
              op, ": mask must be uint8 [n, H/8] bitmask");
  const int* edp = mx_edev_ptr(c10::optional<at::Tensor>(e_dev), x, op);
  TORCH_CHECK(edp != nullptr, op, ": e_dev required");
  auto out = at::empty({a.n, a.H}, w.options());
  auto out8 = at::empty({a.n, a.H}, w.options().dtype(at::kByte));
  if (a.grid == 0) return {out, out8};
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(expand1d_bf16_e5m2_kernel, dim3(a.grid), dim3(256), 0,
                     stream, a.x, a.w, mask.data_ptr<unsigned char>(), edp,
                     (bf16_t*)out.data_ptr(), out8.data_ptr<unsigned char>(),
                     a.n, a.h8);
  return {out, out8};
}

at::Tensor transpose_u8_hip(const at::Tensor& src) {
  TORCH_CHECK(src.is_cuda() && src.dim() == 2 && src.is_contiguous() &&
                  src.scalar_type() == torch::kUInt8,
              "transpose_u8: contiguous 2-d uint8 cuda tensor");
  long long R = src.size(0), C = src.size(1);
  TORCH_CHECK(R % 16 == 0 && C % 16 == 0,
              "transpose_u8 requires rows%16==0 and cols%16==0 (got ", R, "x",
              C, ")");
  TORCH_CHECK((uintptr_t)src.data_ptr() % 16 == 0,
              "transpose_u8: source must be 16-byte aligned");
  auto dst = torch::empty({C, R}, src.options());
  if (R == 0 || C == 0) return dst;
  auto stream = at::cuda::getCurrentCUDAStream();
  dim3 grid((unsigned)((C + TU8_TC - 1) / TU8_TC),
            (unsigned)((R + TU8_TR - 1) / TU8_TR));
  hipLaunchKernelGGL(transpose_u8_kernel, grid, dim3(256), 0, stream,
                     src.data_ptr<unsigned char>(),
                     dst.data_ptr<unsigned char>(), R, C);
  return dst;
}

// the four operand-format pairs of one (epilogue, output type)
template <Epi EPI, bool OUT_FP32>
static void mx_launch_fmt(const MxGemm& g, int64_t a_fmt, int64_t b_fmt) {
  constexpr int E4 = MX_FMT_E4M3, E5 = MX_FMT_E5M2;
  if (a_fmt == E4) {
    if (b_fmt == E4) mx_launch<EPI, false, OUT_FP32, false, E4, E4, true>(g);
    else             mx_launch<EPI, false, OUT_FP32, false, E4, E5, true>(g);
  } else {
    if (b_fmt == E4) mx_launch<EPI, false, OUT_FP32, false, E5, E4, true>(g);
    else             mx_launch<EPI, false, OUT_FP32, false, E5, E5, true>(g);
  }
}

// C[M,N] = 2^(ea+eb) * (A[M,K] . B[N,K]^T) [* bit(mask)], A and B each
// e4m3 (fmt 0) or e5m2 (fmt 1); each exponent is ea (host int) plus the
// int32[1] device tensor ea_dev when given (read in-kernel, clamped to
// the E8M0 range there).  fp32 or bf16 output.
at::Tensor gemm_mx8_nt_fmt_hip(const at::Tensor& a8, int64_t ea,
                               const c10::optional<at::Tensor>& ea_dev,
                               const at::Tensor& b8, int64_t eb,
                               const c10::optional<at::Tensor>& eb_dev,
                               int64_t a_fmt, int64_t b_fmt,
                               const c10::optional<at::Tensor>& mask,
                               bool out_fp32) {
  const char* op = "gemm_mx8_nt_fmt";
  MxGemm g = mx_gemm_operands(op, a8, b8);
  TORCH_CHECK((a_fmt == MX_FMT_E4M3 || a_fmt == MX_FMT_E5M2) &&
                  (b_fmt == MX_FMT_E4M3 || b_fmt == MX_FMT_E5M2),
              op, ": format must be 0 (e4m3) or 1 (e5m2)");
  // host parts stay loud; the device parts are clamped in-kernel
  g.sa = mx_e8m0(op, ea);
  g.sb = mx_e8m0(op, eb);
  g.ea_dev = mx_edev_ptr(ea_dev, a8, op);
  g.eb_dev = mx_edev_ptr(eb_dev, a8, op);
  if (mask.has_value() && mask->defined()) {
    TORCH_CHECK(mask->is_cuda() && mask->is_contiguous() &&
                    mask->scalar_type() == torch::kUInt8 &&
                    mask->numel() == g.M * (g.N / 8),
                op, ": mask must be uint8 [M, N/8] bitmask");
    TORCH_CHECK((uintptr_t)mask->data_ptr() % 8 == 0, op,
                ": mask must be 8-byte aligned");
    g.mask_in = mask->data_ptr<unsigned char>();
  }
  auto opts = a8.options().dtype(out_fp32 ? torch::kFloat : torch::kBFloat16);
  auto C = torch::empty({g.M, g.N}, opts);
  if (g.empty()) return C;
  g.c = C.data_ptr();
  if (g.mask_in) {
    if (out_fp32) mx_launch_fmt<Epi::MaskMul, true>(g, a_fmt, b_fmt);
    else          mx_launch_fmt<Epi::MaskMul, false>(g, a_fmt, b_fmt);
  } else {
    if (out_fp32) mx_launch_fmt<Epi::None, true>(g, a_fmt, b_fmt);
    else          mx_launch_fmt<Epi::None, false>(g, a_fmt, b_fmt);
  }
  return C;
}
