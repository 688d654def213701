// What the MFMA GEMM kernels (gemm.hip, gemm8.hip, gemm_mx8.hip) share
// outside their K-loops: the epilogue of one wave's 64x64 block of C, the
// 16-byte global->LDS load and the accumulator type (the live-row tile test
// is in live_rows.h).
//
// Every kernel gives a wave a 64x64 block = 4x4 fragments of 16x16, fp32
// C/D layout col = lane&15 (fl), row = (lane>>4)*4 + reg (kg = lane>>4);
// the block's origin is (m0 + wm*64, n0 + wn*64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_utils.h"
#include "live_rows.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

enum class Epi {
  None,
  BiasRelu,  // +bias then relu (without HAS_BIAS: relu only)
  MaskMul,   // multiply by a 1-bit ReLU mask (the ReLU backward)
  ReluDot,   // y[row] += sum_col relu(acc + bias[col]) * w3[col]
};

// gemm8.hip's launcher, called from gemm.hip's dispatch
void launch_gemm8(Epi epi, bool has_bias, bool out_fp32, bool emit_mask,
                  const void* ap, const void* bp, const float* bias,
                  const unsigned char* mask, unsigned char* mask_out,
                  void* cp, long long M, long long N, long long K);

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)gsrc,
      (__attribute__((address_space(3))) unsigned int*)lds_dst, 16, 0, 0);
}

// ---- epilogue of one wave's 64x64 block ------------------------------------
// bias, w3: fp32 [N].  mask_in (MaskMul) and mask_out (EMIT_MASK) are 1-bit
// ReLU masks, uint8 [M, N/8], bit e of byte c = column 8c+e > 0.
// ReluDot: C is y (fp32 [M], caller-zeroed) and the [M,N] activation never
// reaches HBM; N is a multiple of 64.  LIVE (ReluDot only): rows of the tile
// at or past live_rows add nothing to y, whatever their A rows hold.
// WHOLE_STRIPES: the caller's N is a multiple of 64, so the byte-wise mask
// gather of an edge stripe is not compiled in.
template <Epi EPI, bool HAS_BIAS, bool OUT_FP32, bool EMIT_MASK = false,
          bool LIVE = false, bool WHOLE_STRIPES = false>
__device__ __forceinline__ void tile_epilogue(
    f32x4 (&acc)[4][4], const float* __restrict__ bias,
    const float* __restrict__ w3, const unsigned char* __restrict__ mask_in,
    unsigned char* __restrict__ mask_out, void* __restrict__ C, long long M,
    long long N, long long m0, long long n0, int wm, int wn, int fl, int kg,
    int live_rows = 0) {
  if (EPI == Epi::ReluDot) {
    // per (i,r) row: 16 lanes (fl) x 4 j-frags hold the wave's 64-column
    // strip; butterfly-reduce across fl, then the fl==0 lane of each kg row
    // atomically adds its wave's partial (every wave along N adds to the
    // same row; the caller adds the b3 offset)
    float w3v[4], b2v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long long col = n0 + wn * 64 + j * 16 + fl;
      w3v[j] = w3[col];
      b2v[j] = HAS_BIAS ? bias[col] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          part = fmaf(fmaxf(acc[i][j][r] + b2v[j], 0.0f), w3v[j], part);
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
          part += __shfl_xor(part, m, 64);  // reduce across fl (lane&15)
        // LIVE: a 32-bit compare of the row's place in the tile
        if (fl == 0 &&
            (!LIVE || wm * 64 + i * 16 + kg * 4 + r < live_rows)) {
          long long row = m0 + wm * 64 + i * 16 + kg * 4 + r;
          atomicAdd((float*)C + row, part);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // MaskMul: one aligned u64 per row covers this wave's whole 64-col
    // stripe (bit b = col n0+wn*64+b; replaces 16 scalar byte loads), read
    // here, after the accumulators are final
    unsigned long long mrow[4];
    if (EPI == Epi::MaskMul && WHOLE_STRIPES) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long long row = m0 + wm * 64 + i * 16 + kg * 4 + r;
        mrow[r] = row < M ? *(const unsigned long long*)(mask_in +
                                                         row * (N >> 3) +
                                                         ((n0 + wn * 64) >> 3))
                          : 0ull;
      }
    } else if (EPI == Epi::MaskMul) {
      const long long stripe = n0 + wn * 64;
      const bool full = stripe + 64 <= N;  // edge tile: byte-wise gather
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long long row = m0 + wm * 64 + i * 16 + kg * 4 + r;
        if (row >= M) {
          mrow[r] = 0ull;
        } else if (full) {
          mrow[r] = *(const unsigned long long*)(mask_in + row * (N >> 3) +
                                                 (stripe >> 3));
        } else {
          unsigned long long v = 0;
          for (int b8 = 0; b8 < 8; ++b8)
            if (stripe + b8 * 8 < N)
              v |= (unsigned long long)
                       mask_in[row * (N >> 3) + ((stripe >> 3) + b8)]
                   << (8 * b8);
          mrow[r] = v;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long long col = n0 + wn * 64 + j * 16 + fl;
      bool col_ok = col < N;
      float bval =
          (EPI == Epi::BiasRelu && HAS_BIAS && col_ok) ? bias[col] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long long row = m0 + wm * 64 + i * 16 + kg * 4 + r;
        bool row_ok = row < M;
        float v = acc[i][j][r];
        if (EPI == Epi::BiasRelu) {
          v += bval;
          v = fmaxf(v, 0.0f);
        } else if (EPI == Epi::MaskMul) {
          v = (mrow[r] >> (j * 16 + fl)) & 1 ? v : 0.0f;
        }
        if (EMIT_MASK) {
          // wave-wide ballot OUTSIDE the row/col conditional; lane
          // kg*16+fl holds (row of kg, col fl), so each kg group's 16-bit
          // slice is two consecutive mask bytes of its row
          unsigned long long bal = __ballot(v > 0.0f);
          if (fl == 0 && row_ok && col < N) {
            unsigned short bits =
                (unsigned short)((bal >> (kg * 16)) & 0xFFFF);
            *(unsigned short*)(mask_out + row * (N >> 3) + (col >> 3)) = bits;
          }
        }
        if (row_ok && col_ok) {
          if (OUT_FP32)
            ((float*)C)[row * N + col] = v;
          else
            ((bf16_t*)C)[row * N + col] = f32_to_bf16(v);
        }
      }
    }
  }
}
