"""csrc/batchnorm_live_index.h -- the row arithmetic of the live-frame BatchNorm, padding and row-zeroing kernels -- compiled with the
host compiler and swept: all (Lx, live) with Lx <= 9 and live in -2 .. Lx + 3, three batch sizes.  The clamp, the liveness of every
physical row, and the live row count B * clamp(live) (the statistics' divisor), each against the plain statement written here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEP = r"""
#include <cstdio>
#include "batchnorm_live_index.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d) B=%d Lx=%d live=%d r=%d\n", #c, __LINE__, B, Lx, live, r); return 1; } } while (0)
int main() {
  int B = 0, Lx = 0, live = 0, r = 0;
  long long cases = 0;
  for (B = 1; B <= 3; ++B) for (Lx = 1; Lx <= 9; ++Lx) for (live = -2; live <= Lx + 3; ++live) {
    r = -1;
    const long long want = live < 0 ? 0 : (live > Lx ? Lx : live);
    const long long c = bnl_clamp(live, Lx);
    CHECK(c == want && c >= 0 && c <= Lx);
    long long n = 0;
    for (r = 0; r < B * Lx; ++r) {
      const int t = r - (r / Lx) * Lx;
      CHECK(bnl_row_live(r, Lx, c) == (t < want));
      n += bnl_row_live(r, Lx, c) ? 1 : 0;
    }
    r = -1;
    CHECK(n == (long long)B * want);
    CHECK(bnl_live_rows((long long)B * Lx, Lx, c) == n);
    if (live == Lx) CHECK(n == (long long)B * Lx);       // nothing is dead: the variant is the plain kernel
    ++cases;
  }
  // values of the cell that do not fit the row count's type on the way in; a row index past 2^31
  B = 1; Lx = 7; r = -1;
  live = 2147483647; CHECK(bnl_clamp(live, Lx) == 7);
  live = -2147483647 - 1; CHECK(bnl_clamp(live, Lx) == 0);
  CHECK(bnl_row_live((1LL << 33) + 2, 1LL << 32, 3) && !bnl_row_live((1LL << 33) + 3, 1LL << 32, 3));
  CHECK(bnl_live_rows(3LL << 32, 1LL << 32, 5) == 15);
  std::printf("OK %lld cases\n", cases);
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_live_index_header_sweep_on_the_host(tmp_path):
    src = tmp_path / "sweep.cpp"
    src.write_text(SWEEP)
    exe = tmp_path / "sweep"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "speecht5_amd", "csrc"), str(src),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    assert r.stdout.split()[1] == str(3 * sum(Lx + 6 for Lx in range(1, 10)))
