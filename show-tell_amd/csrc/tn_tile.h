// LDS image of the token-contraction GEMM (csrc/gemm_tn.hip): index arithmetic only, host and device, so that
// tests/test_tn_tile_map.py can check it on the CPU against the documented semantics of ds_read_b64_tr_b16.
//
// One image holds TN_BK consecutive rows (tokens) of a [K][cols] bf16 operand as they lie in memory: TN_COLS = 128 columns
// (256 bytes) per row, in 16-byte chunks.  Chunk ch of row `row` sits at chunk position ch ^ swz(row) of that row.  The same
// image serves the A and the B side: both are read column-wise (the contraction index is the ROW of both operands).
//
// A 16x16x32 MFMA operand for columns 16*c16 .. 16*c16 + 15 of the image takes two transposed reads (half h = 0, 1).  In each
// 16-lane group g = lane >> 4, lane 4q + p supplies the address of row 8g + 4h + q, columns 16*c16 + 4p .. + 3, and lane i
// receives column 16*c16 + i of those four rows: element j = 4h + q of its fragment is image[8g + j][16*c16 + i], which is
// the operand map of v_mfma_f32_16x16x32_bf16 (k = 8 * (lane >> 4) + j, row or column = lane & 15).
//
// Banks: a 32-lane half (two groups) reads rows {8g + 4h + q} for two values of g and q = 0..3, 32 bytes each, from the same
// chunk pair 2*c16, 2*c16 + 1.  swz(row) >> 1 = 2 * (row & 3) + ((row >> 3) & 1) is different for those eight rows, so the
// eight 32-byte pieces fall on eight different pairs of a 256-byte bank row: no conflict.  A 16-byte store of 8 consecutive
// lanes (chunks 8u .. 8u + 7 of one row) lands on 8 different chunks modulo 8: no conflict under the 32-bank rule of stores.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TN_HD __host__ __device__ __forceinline__
#else
#define TN_HD inline
#endif

constexpr int TN_BK = 32;                 // rows of one image = K of one v_mfma_f32_16x16x32_bf16
constexpr int TN_COLS = 128;              // columns of one image = one output tile edge
constexpr int TN_ROW_BYTES = 2 * TN_COLS;
constexpr int TN_IMAGE_BYTES = TN_BK * TN_ROW_BYTES;

TN_HD int tn_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// byte offset of 16-byte chunk ch (0..15) of row `row` (0..TN_BK-1): the address the tile loader stores to
TN_HD int tn_store_off(int row, int ch) { return TN_ROW_BYTES * row + 16 * (ch ^ tn_swz(row)); }

// row of the image whose address `lane` supplies for half h of a fragment
TN_HD int tn_read_row(int lane, int h) { return 8 * (lane >> 4) + 4 * h + ((lane & 15) >> 2); }

// byte address `lane` hands to ds_read_b64_tr_b16 for half h of the fragment of columns 16*c16 .. 16*c16 + 15
TN_HD int tn_read_off(int lane, int c16, int h) {
  const int p = lane & 3;
  return tn_store_off(tn_read_row(lane, h), 2 * c16 + (p >> 1)) + 8 * (p & 1);
}
