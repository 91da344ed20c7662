// Host sweep of speecht5_amd/csrc/ctc_pack_index.h: rows walked exactly as ctc_pack_rows_kernel (csrc/ctc_loss.hip) walks them -- one
// wave per row, chunks of CP_WAVE columns, one ballot per chunk, a running base, then the tail fill -- against a plain loop.
// Checked for every row: the kept entries land in order from column 0; every column of the output row is written exactly once;
// no destination leaves the row; kept and total are the plain counts.  Build with the host compiler and the address and
// undefined-behaviour sanitizers and run it directly (`make -C speecht5_amd/csrc ctc_pack_sweep`):
//   g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -I speecht5_amd/csrc tools/ctc_pack_sweep.cpp
// -DPLANT_INCLUSIVE (an inclusive prefix popcount) and -DPLANT_TAIL_FROM_CHUNK (a tail fill that starts at the next chunk boundary)
// are planted faults the sweep must catch (tests/test_ctc_pack_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ctc_pack_index.h"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d) B=%lld L=%lld row=%lld\n", #cond, __LINE__, B, L, b); return 1; } } while (0)

static long long lane_dest(long long base, uint64_t ballot, int lane) {
#ifdef PLANT_INCLUSIVE
  return cp_lane_dest(base, ballot, lane + 1);
#else
  return cp_lane_dest(base, ballot, lane);
#endif
}

static long long tail_first(long long kept, int lane) {
#ifdef PLANT_TAIL_FROM_CHUNK
  return cp_tail_first((kept + CP_WAVE - 1) / CP_WAVE * CP_WAVE, lane);
#else
  return cp_tail_first(kept, lane);
#endif
}

int main() {
  const long long PAD = 1, EOS = 2;
  const long long Ls[] = {1, 2, 3, 7, 63, 64, 65, 127, 128, 129, 200, 257, 600, 1909};
  const long long Bs[] = {1, 2, 3, 4, 5, 7, 9};
  unsigned r = 2024u;
  long long rows = 0, B = 0, L = 0, b = 0;
  CHECK(cp_check(0, 0) == 0 && cp_check(-1, 4) == 1 && cp_check(4, -1) == 1 && cp_check(1LL << 31, 1) == 1 && cp_check(1, 1LL << 31) == 1);
  CHECK(cp_chunks(0) == 0 && cp_chunks(-3) == 0 && cp_chunks(1) == 1 && cp_chunks(64) == 1 && cp_chunks(65) == 2);
  CHECK(cp_lane_dest(5, ~0ull, 0) == 5 && cp_lane_dest(5, ~0ull, 63) == 68 && cp_next_base(5, ~0ull) == 69 && cp_next_base(5, 0) == 5);
  for (long long Bi : Bs) for (long long Li : Ls) {
    B = Bi; L = Li;
    std::vector<long long> target((size_t)(B * L)), packed((size_t)(B * L), -77), offsets((size_t)B, -77), kept((size_t)B, -77);
    std::vector<int> writes((size_t)(B * L), 0);
    for (b = 0; b < B; ++b) {
      // row kinds in turn: all pad, eos only, full without pad or eos, label + eos + pad, eos in mid-row, random mixture
      const int kind = (int)((b + Li) % 6);
      r = r * 1664525u + 1013904223u;
      const long long n = kind == 2 ? L : (long long)((r >> 8) % (unsigned)L);
      for (long long i = 0; i < L; ++i) {
        r = r * 1664525u + 1013904223u;
        long long v = 4 + (r >> 10) % 70;
        if (kind == 0) v = PAD;
        else if (kind == 1) v = i == 0 ? EOS : PAD;
        else if (kind == 3) v = i < n ? v : (i == n ? EOS : PAD);
        else if (kind == 4) v = i == L / 2 ? EOS : v;
        else if (kind == 5) v = (r >> 20) % 4 == 0 ? PAD : ((r >> 20) % 4 == 1 ? EOS : v);
        target[(size_t)(b * L + i)] = v;
      }
    }
    long long wave_total[CP_WAVES] = {0};
    for (int wave = 0; wave < CP_WAVES; ++wave)
      for (b = wave; b < B; b += CP_WAVES) {
        const long long row = cp_offset(b, L);
        CHECK(row == b * L);
        long long base = 0;
        for (long long c = 0; c < cp_chunks(L); ++c) {
          uint64_t ballot = 0;
          for (int lane = 0; lane < CP_WAVE; ++lane) {
            const long long col = cp_column(c, lane);
            if (col < L && cp_keep(target[(size_t)(row + col)], PAD, EOS)) ballot |= 1ull << lane;
          }
          for (int lane = 0; lane < CP_WAVE; ++lane) {
            if (!((ballot >> lane) & 1ull)) continue;
            const long long d = lane_dest(base, ballot, lane);
            CHECK(d >= 0 && d < L && d <= cp_column(c, lane));     // inside the row, never behind the column it came from
            packed[(size_t)(row + d)] = target[(size_t)(row + cp_column(c, lane))];
            ++writes[(size_t)(row + d)];
          }
          base = cp_next_base(base, ballot);
        }
        for (int lane = 0; lane < CP_WAVE; ++lane)
          for (long long col = tail_first(base, lane); col < L; col += CP_WAVE) {
            CHECK(col >= base && col < L);
            packed[(size_t)(row + col)] = PAD;
            ++writes[(size_t)(row + col)];
          }
        offsets[(size_t)b] = row;
        kept[(size_t)b] = base;
        wave_total[wave] += base;
        ++rows;
      }
    long long total = 0, want_total = 0;
    for (int w = 0; w < CP_WAVES; ++w) total += wave_total[w];
    for (b = 0; b < B; ++b) {
      long long k = 0;
      for (long long i = 0; i < L; ++i) {
        const long long v = target[(size_t)(b * L + i)];
        if (v != PAD && v != EOS) { CHECK(packed[(size_t)(b * L + k)] == v); ++k; }
      }
      for (long long i = k; i < L; ++i) CHECK(packed[(size_t)(b * L + i)] == PAD);
      for (long long i = 0; i < L; ++i) CHECK(writes[(size_t)(b * L + i)] == 1);
      CHECK(kept[(size_t)b] == k && offsets[(size_t)b] == b * L);
      want_total += k;
    }
    b = -1;
    CHECK(total == want_total);
  }
  std::printf("OK %lld rows\n", rows);
  return 0;
}
