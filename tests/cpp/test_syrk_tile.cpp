// LDS bank arithmetic of k_buildp's SYRK tile (kalibr_amd/csrc/kb_syrk_tile.h) on the CPU, with the index function the
// kernel uses.  gfx950's rules for 8-byte accesses, byte address a:
//   ds_read_b64:  two 32-lane groups {0-31}, {32-63}, bank = (a / 4) mod 64
//   ds_write_b64: four contiguous 16-lane groups, bank = (a / 4) mod 32
// A group is conflict-free when no bank is touched by two distinct addresses; an 8-byte access touches the bank pair
// a / 4, a / 4 + 1 (a is 8-byte aligned), so distinct pairs suffice.
// usage: test_syrk_tile [stride17]   (stride17: the same counts for the 17-double row stride, printed, not asserted)
#include <cstdio>
#include <cstring>
#include <set>

#include "../../kalibr_amd/csrc/kb_syrk_tile.h"

static_assert(kb_tile::idx(0, 0) == 0 && kb_tile::idx(63, 0) == 63 && kb_tile::idx(5, 3) == 3 * 66 + 5, "by columns");

// the worst number of distinct addresses on one bank pair within any lane group (1 = conflict-free)
template <class F>
static int worst(int group, int banks, F addr_of_lane) {
  int w = 0;
  for (int g0 = 0; g0 < 64; g0 += group) {
    int cnt[64] = {0};
    std::set<int> seen;
    for (int l = g0; l < g0 + group; ++l) {
      const int a = 8 * addr_of_lane(l);
      if (!seen.insert(a).second) continue;  // identical addresses broadcast
      const int b = (a / 4) % banks;
      cnt[b]++;
      cnt[(b + 1) % banks]++;
    }
    for (int b = 0; b < banks; ++b) w = cnt[b] > w ? cnt[b] : w;
  }
  return w;
}

int main(int argc, char** argv) {
  const bool s17 = argc > 1 && !strcmp(argv[1], "stride17");
  auto idx = [&](int row, int col) { return s17 ? row * 17 + col : kb_tile::idx(row, col); };
  int bad = 0;
  // injective over 64 x 16, inside the 64 x 17 doubles the launch layout allots
  std::set<int> all;
  for (int r = 0; r < 64; ++r)
    for (int c = 0; c < 16; ++c) {
      const int i = idx(r, c);
      if (i < 0 || i >= 64 * 17 || !all.insert(i).second) {
        printf("index (%d, %d) -> %d repeated or out of range\n", r, c, i);
        bad++;
      }
    }
  // the operand reads: pair p, quad 0 / 1
  int wr = 0, ww = 0;
  for (int p = 0; p < 8; ++p)
    for (int quad = 0; quad < 2; ++quad) {
      const int w = worst(32, 64, [&](int l) {
        return s17 ? idx(8 * p + 4 * quad + (l >> 4), l & 15) : kb_tile::read_idx(p, quad, l);
      });
      if (!s17 && kb_tile::read_idx(p, quad, 37) != kb_tile::idx(8 * p + 4 * quad + 2, 5)) bad++;
      wr = w > wr ? w : wr;
      if (w != 1 && !s17) {
        printf("read p=%d quad=%d: %d-way\n", p, quad, w);
        bad++;
      }
    }
  // the 16 column stores, row = lane
  for (int q = 0; q < 16; ++q) {
    const int w = worst(16, 32, [&](int l) { return s17 ? idx(l, q) : kb_tile::store_idx(l, q); });
    ww = w > ww ? w : ww;
    if (w != 1 && !s17) {
      printf("store q=%d: %d-way\n", q, w);
      bad++;
    }
  }
  printf("%d %d %d\n", wr, ww, (int)all.size());
  return bad ? 1 : 0;
}
