// Host check of csrc/tn_tile.h, the LDS index arithmetic of the token-contraction GEMM (built and run by test_tn_tile_map.py with
// -fsanitize=address,undefined).  It fills an emulated LDS image through tn_store_off, performs ds_read_b64_tr_b16 as documented
// (per 16-lane group, lane 4q + p supplies the address of row q, columns 4p .. 4p + 3 of a 4 x 16 block; lane i receives column i,
// row q in element q) at the addresses of tn_read_off, and compares what every lane holds with the operand map of
// v_mfma_f32_16x16x32_bf16: element j of lane l is [k = 8 (l >> 4) + j][column l & 15].  Then it counts bank conflicts: reads by
// 32-lane halves over 64 banks, 16-byte stores by groups of 8 consecutive lanes over 32 banks; an access costs, per group, the
// largest number of distinct dwords on one bank, and every cycle beyond the first is a conflict.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "tn_tile.h"

static int fails = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++fails <= 20) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } } } while (0)

static uint16_t code(int row, int col) { return (uint16_t)(row * TN_COLS + col); }

// extra cycles of one lane group: `width` dwords per lane starting at byte address a[i]
static int extra_cycles(const std::vector<int>& a, int width, int banks) {
  std::vector<std::set<int>> on(banks);
  for (int addr : a)
    for (int w = 0; w < width; ++w) on[(addr / 4 + w) % banks].insert(addr / 4 + w);
  size_t worst = 1;
  for (const auto& s : on) worst = s.size() > worst ? s.size() : worst;
  return (int)worst - 1;
}

template <typename ReadOff>
static int read_conflicts(ReadOff off) {
  int total = 0;
  for (int c16 = 0; c16 < TN_COLS / 16; ++c16)
    for (int h = 0; h < 2; ++h)
      for (int half = 0; half < 2; ++half) {
        std::vector<int> a;
        for (int l = 32 * half; l < 32 * half + 32; ++l) a.push_back(off(l, c16, h));
        total += extra_cycles(a, 2, 64);
      }
  return total;
}

int main() {
  // the loader's stores cover the image exactly once, 16-byte aligned
  std::vector<uint16_t> img(TN_IMAGE_BYTES / 2, 0xffff);
  std::vector<int> hit(TN_IMAGE_BYTES / 16, 0);
  for (int row = 0; row < TN_BK; ++row)
    for (int ch = 0; ch < TN_COLS / 8; ++ch) {
      const int o = tn_store_off(row, ch);
      EXPECT(o % 16 == 0 && o >= 0 && o + 16 <= TN_IMAGE_BYTES, "store offset %d of (row %d, chunk %d)", o, row, ch);
      if (o % 16 != 0 || o < 0 || o + 16 > TN_IMAGE_BYTES) continue;
      ++hit[o / 16];
      for (int e = 0; e < 8; ++e) img[o / 2 + e] = code(row, 8 * ch + e);
    }
  for (int v : hit) EXPECT(v == 1, "a 16-byte slot is stored %d times", v);

  // every lane of every operand fragment of the 128-column image (the one tile shape gemm_tn_kernel instantiates)
  for (int c16 = 0; c16 < TN_COLS / 16; ++c16)
    for (int h = 0; h < 2; ++h) {
      int addr[64];
      for (int l = 0; l < 64; ++l) {
        addr[l] = tn_read_off(l, c16, h);
        EXPECT(addr[l] % 8 == 0, "lane %d: address %d not 8-byte aligned", l, addr[l]);
        EXPECT(addr[l] >= 0 && addr[l] + 8 <= TN_IMAGE_BYTES, "lane %d: address %d outside the image", l, addr[l]);
        if (addr[l] % 8 != 0 || addr[l] < 0 || addr[l] + 8 > TN_IMAGE_BYTES) return 1;
      }
      for (int g = 0; g < 4; ++g) {
        uint16_t block[4][16];
        for (int q = 0; q < 4; ++q)
          for (int p = 0; p < 4; ++p)
            for (int e = 0; e < 4; ++e) block[q][4 * p + e] = img[addr[16 * g + 4 * q + p] / 2 + e];
        for (int i = 0; i < 16; ++i)
          for (int q = 0; q < 4; ++q) {
            const int l = 16 * g + i, j = 4 * h + q;
            const uint16_t want = code(8 * (l >> 4) + j, 16 * c16 + (l & 15));
            EXPECT(block[q][i] == want, "fragment c16=%d lane %d element %d holds (%d, %d), wants (%d, %d)", c16, l, j,
                   block[q][i] / TN_COLS, block[q][i] % TN_COLS, want / TN_COLS, want % TN_COLS);
          }
      }
    }

  const int rd = read_conflicts([](int l, int c16, int h) { return tn_read_off(l, c16, h); });
  // the same reads on plain 256-byte rows (no chunk XOR): the eight rows of a half share their banks, and the counter must see it
  const int rd_plain = read_conflicts([](int l, int c16, int h) {
    return TN_ROW_BYTES * tn_read_row(l, h) + 32 * c16 + 8 * (l & 3);
  });
  // stores: thread t of 256 writes chunk t & 15 of rows (t >> 4) and (t >> 4) + 16
  int wr = 0;
  for (int t0 = 0; t0 < 256; t0 += 8)
    for (int i = 0; i < 2; ++i) {
      std::vector<int> a;
      for (int t = t0; t < t0 + 8; ++t) a.push_back(tn_store_off((t >> 4) + 16 * i, t & 15));
      wr += extra_cycles(a, 4, 32);
    }
  std::printf("tile %dx%d read_conflicts=%d write_conflicts=%d plain_read_conflicts=%d\n", TN_BK, TN_COLS, rd, wr, rd_plain);
  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
